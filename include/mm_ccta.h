/*
 * mm_ccta.h -- C ABI of the CCTA diameter search: 41 radial scalings of a
 * vessel region scored by the symmetric RMS nearest-neighbour distance to a reference cloud, in
 * 3-D; and of the CCTA mesh labelling that produces the regions it scales (aorta / RCA / LCA,
 * with occlusion removal by ray casting at an acute take-off).  Same conventions as
 * mm_hausdorff.h.  Points are xyz triples (f64), caller-owned.
 *
 * Reference interfaces replaced (paths relative to the reference checkout):
 *   src/ccta/adjust_mesh/scale_coronary.rs:8-63     centerline_based_wall_diameter_optimization
 *   src/ccta/adjust_mesh/scale_coronary.rs:65-88    centerline_based_aortic_diameter_optimization
 *   src/ccta/adjust_mesh/scale_coronary.rs:90-131   centerline_based_diameter_optimization
 *   src/ccta/adjust_mesh/scale_coronary.rs:133-183  find_region_points
 *   src/ccta/adjust_mesh/scale_coronary.rs:188-216  symmetric_nn_distance
 *   src/ccta/adjust_mesh/scale_coronary.rs:218-261  centerline_based_diameter_morphing
 *   src/ccta/adjust_mesh/scale_coronary.rs:263-340  find_points_by_cl_region_rs, find_cl_points_in_range
 *   src/ccta/adjust_mesh/scale_coronary.rs:342-409  clean_up_non_section_points
 *   src/ccta/adjust_mesh/label_coronary.rs:29-197  ray_triangle_intersection, remove_occluded_points_ray_triangle_rust
 *   src/ccta/adjust_mesh/label_coronary.rs:201-289 find_centerline_bounded_points, find_faces_near_points
 *   src/ccta/adjust_mesh/label_coronary.rs:296-640 find_aortic_points, final_reclassification
 *   src/ccta/discretizing/projecting.rs:13-200       walk_centerline_slices, voronoi_partition, project_to_plane
 *   src/ccta/discretizing/resampling.rs:11-229       create_uniform_contours, resample_spline
 *   src/ccta/discretizing.rs:13-22, discretizing/vessel_tree.rs:21-83  discretize_vessel_rs, from_results_dict
 *   src/ccta/binding/ccta_py.rs:541-580, label_coronary.rs:428-455  keep_largest_connected_component
 *   multimodars/ccta/labeling.py:415-487           label_branches
 *   multimodars/ccta/fixing_functions.py:13-49     manual_hole_fill
 *   multimodars/ccta/__init__.py:432-499           create_wall_mesh (composed in Python from the pieces here)
 *   src/ccta/binding/ccta_py.rs:743-814            smooth_mesh_labels
 *   multimodars/ccta/fixing_functions.py:196-219   checksurfdist / maxsurfdist (measured here: mm_point_mesh_distance)
 * Python entry points that bind them: src/ccta/binding/ccta_py.rs:52-481, 724-920 (discretize_vessel,
 * discretize_vessel_tree)
 * (find_centerline_bounded_points_simple, remove_occluded_points_ray_triangle, find_faces_near_points,
 * find_aortic_points, final_reclassification, adjust_diameter_centerline_morphing_simple,
 * find_proximal_distal_scaling, find_aortic_scaling, find_aortic_wall_scaling), wrapped by
 * multimodars/ccta/labeling.py (label_geometry) and multimodars/ccta/scaling.py.
 *
 * All nearest-neighbour minima are computed on the device in exact f64 (mm_nn_kernels.hip); the
 * per-point minima are summed on the host in index order (the reference's rayon sum has no fixed
 * order; the sequential one is among those it can produce).  The labelling's ray-triangle tests run
 * on the device in exact f64 (mm_ray_kernels.hip); its radius queries use the same exact radius
 * counts as mm_clean_outlier_points; the bookkeeping on adjacency graphs is host C++.  The vessel discretisation's
 * nearest-anchor assignment and plane projection run on the device in exact f64 (mm_slice_kernels.hip); its anchors
 * and spline resampling are host f64.  The mesh morphing's nearest-centerline search and radial move run on the device
 * in exact f64 (mm_morph_kernels.hip).  The mesh trimming's face membership, open-edge counting and compaction run on the
 * device (mm_trim_kernels.hip); its ring logic on the rim is host C++.  The branch labelling's membership masks are one device
 * pass in exact f64 (mm_branch_kernels.hip); its lists are read off the masks on the host.
 * The mesh closing's edge table, winding, open half-edges, fans, volume and label votes run on the device
 * (mm_weld_kernels.hip, mm_close_kernels.hip); its walk over the rim is host C++.
 * The surface distance's point-to-triangle minima, winning faces and closest points are computed on the device in exact
 * f64 (mm_tri_kernels.hip); the staging order and the pruning bounds are host C++, its means are summed in Python.
 */
#ifndef MM_CCTA_H
#define MM_CCTA_H

#include "mm_centerline.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MM_CCTA_SCALING_STEPS 41   /* -2.0 .. 2.0 mm in steps of 0.1 (scale_coronary.rs:70-73) */

/* min_p |q - p|^2 for every query q of every (query set, point set) pair.  Sets: n_sets CSR ranges
 * of xyz triples; pair k reads sets q_set[k] / p_set[k] and writes sets[q_set[k]].n values at
 * out + out_off[k].  An empty point set yields +inf. */
int     mm_nn_min_sq_batch(mm_engine* e, int n_sets, const int64_t* set_off, const double* xyz,
                           int n_pairs, const int32_t* q_set, const int32_t* p_set,
                           const int64_t* out_off, double* out);
/* TEST HOOK (nothing in the product calls it; no engine, no device): the host side of one nearest-neighbour batch
 * (mm_nn_min_sq_batch, the scaling searches) and of one radius count (mm_clean_outlier_points), as their launch paths build
 * it.  Sets: n_sets CSR ranges of xyz triples; a set with derived[s] != 0 (derived nullable) is its base points moved by
 * adj[s] along unit (triples) where has (one flag per point) is set, as the scaling searches' morphed copies.
 * order_like (nullable, one entry per set): the set whose staging order this one shares.  Pairs: q_set[k] / p_set[k].
 * perm (one entry per point, by set_off): staged position j of set s holds its original point perm[set_off[s] + j]
 * (the identity where a set is staged as given).  items (5 int32 each: list 0 = pass A of k_nn3_min, 1 = pass B,
 * 2 = k_nn3_count for the squared radius r2; caller's pair; first staged query q0; first point c0; chunks) and item_lb2
 * (the item's lower bound of the squared distance between its queries' and points' boxes) receive at most cap items,
 * lists in that order.  info[6] = {items of pass A, of pass B, of the count, queries per block, points per chunk,
 * chunks per unpruned item}. */
int     mm_nn_plan(int n_sets, const int64_t* set_off, const double* xyz, const double* unit, const uint8_t* has,
                   const uint8_t* derived, const double* adj, const int32_t* order_like, int n_pairs, const int32_t* q_set,
                   const int32_t* p_set, double r2, int32_t* perm, int64_t* info, int32_t* items, double* item_lb2,
                   int64_t cap);
/* symmetric_nn_distance (:188-216); +inf if either set is empty */
int     mm_symmetric_nn_distance(mm_engine* e, const double* a_xyz, int64_t na, const double* b_xyz, int64_t nb,
                                 double* out);
/* centerline_based_diameter_morphing (:218-261), host f64 */
int     mm_diameter_morphing(const mm_clpoint* cl, int64_t ncl, const double* pts_xyz, int64_t n,
                             double diameter_adjustment_mm, double* out_xyz);
/* find_region_points (:133-183): selected (nearest n_points, sorted by distance then index) and
 * remaining (input order); buffers hold n triples each.  Returns the number selected. */
int64_t mm_find_region_points(mm_engine* e, const double* anomalous_xyz, int64_t n, const double* reference_xyz,
                              int64_t nr, int64_t n_points, double* selected_xyz, double* remaining_xyz);
/* centerline_based_aortic_diameter_optimization (:65-88).  all_dist (nullable) receives the
 * MM_CCTA_SCALING_STEPS distances.  *best = f64::MAX if every distance is +inf (empty input). */
int     mm_aortic_diameter_optimization(mm_engine* e, const double* intramural_xyz, int64_t ni,
                                        const double* reference_xyz, int64_t nr, const mm_clpoint* cl, int64_t ncl,
                                        double* best, double* all_dist);
/* centerline_based_diameter_optimization (:90-131) */
int     mm_diameter_optimization(mm_engine* e, const double* anomalous_xyz, int64_t n, int64_t n_proximal,
                                 int64_t n_distal, const mm_clpoint* cl, int64_t ncl,
                                 const double* proximal_reference_xyz, int64_t npr,
                                 const double* distal_reference_xyz, int64_t ndr,
                                 double* proximal_best, double* distal_best);
/* centerline_based_wall_diameter_optimization (:8-63), host f64 */
int     mm_wall_diameter_optimization(const mm_clpoint* cl, int64_t ncl, const double ref_pt[3],
                                      const double* aortic_xyz, int64_t na, double* out);

/* clean_up_non_section_points (:342-409; Python: clean_outlier_points, ccta_py.rs:345-358): for every point of
 * `cleanup`, the neighbours within neighborhood_radius among the reference points and among the other cleanup
 * points are counted on the device (exact f64, |q - p|^2 <= r^2 like rstar's locate_within_distance);
 * to_reference[i] = 1 where ref / (ref + self) >= min_neighbor_ratio: the point joins the reference set
 * (appended in input order), 0: it stays. */
int     mm_clean_outlier_points(mm_engine* e, const double* cleanup_xyz, int64_t nc, const double* reference_xyz,
                                int64_t nr, double neighborhood_radius, double min_neighbor_ratio,
                                uint8_t* to_reference);
/* find_points_by_cl_region_rs (:263-312; Python: find_points_by_cl_region, ccta_py.rs:304-319).  cl_frame_index
 * (nullable -> 0, 1, 2, ...) = contour_point.frame_index of every centerline point.  label[i]:
 *   0 proximal, 1 distal, 2 between (anomalous section), 3 proximal moved to between by the first clean-up,
 *   4 distal moved to between by the second.  The reference's three vectors are: proximal = labels 0 in input
 *   order; distal = labels 1 in input order; between = labels 2 in input order, then 3 in input order, then 4. */
int     mm_find_points_by_cl_region(mm_engine* e, const mm_clpoint* cl, const uint32_t* cl_frame_index, int64_t ncl,
                                    const double* frame_centroids_xyz, int64_t n_frames, const double* points_xyz,
                                    int64_t n, uint8_t* label);

/* ---- mesh labelling (label_coronary.rs).  Flag outputs: the caller selects the points. ---------------------------- */

/* find_centerline_bounded_points (:201-235): inside[i] = 1 iff some centerline point lies within squared distance
 * <= radius * radius of point i.  Returns the number inside; an empty point set or centerline is MM_ERR_INVALID
 * (the reference's Err, :206-209). */
int64_t mm_centerline_bounded_points(mm_engine* e, const mm_clpoint* cl, int64_t ncl, const double* pts_xyz, int64_t n,
                                     double radius, uint8_t* inside);
/* find_faces_near_points (:242-289): a vertex matches iff some point lies within squared distance <= tol * tol;
 * face_selected[f] = 1 iff a corner of face f matches.  faces: nf index triples into vertices; an index out of range
 * is MM_ERR_INVALID.  Returns the number of faces selected (0 if any input is empty). */
int64_t mm_faces_near_points(mm_engine* e, const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf,
                             const double* pts_xyz, int64_t n, double tol, uint8_t* face_selected);
/* remove_occluded_points_ray_triangle_rust (:70-197).  tri: nf triangles of 9 doubles (v0, v1, v2).  Rays run from
 * every aortic centerline point to the coronary points take(ceil(range_mm / s)).step_by(ceil(step_size_mm / s)), s
 * the mean of the two centerlines' mean spacings (Rust's saturating casts); a ray that hits at least 3 faces excludes
 * the one of smallest t (ties: lowest index).  removed[i] = 1 iff a vertex of an excluded face lies within squared
 * distance <= 0.5 of point i; face_excluded (nullable) receives the excluded faces.  Returns the number removed.
 * Empty points, faces or aortic centerline: nothing removed; a step of 0 points: MM_ERR_INVALID (a panic there). */
int64_t mm_occluded_points(mm_engine* e, const mm_clpoint* cl_coronary, int64_t ncc, const mm_clpoint* cl_aorta,
                           int64_t nca, double range_mm, const double* pts_xyz, int64_t n, const double* tri,
                           int64_t nf, double step_size_mm, uint8_t* removed, uint8_t* face_excluded);
/* find_aortic_points (:296-313), host: keep[i] = 1 iff vertex i is bit-for-bit in neither a nor b.  Returns the
 * number kept. */
int64_t mm_find_aortic_points(const double* vertices_xyz, int64_t nv, const double* a_xyz, int64_t na,
                              const double* b_xyz, int64_t nb, uint8_t* keep);
/* final_reclassification (:337-640), host.  label[v]: 0 aorta, 1 rca, 2 lca, 3 rca removed, 4 lca removed.  Points
 * are matched to vertices by bit pattern (the last of duplicated vertices wins) and applied in the order rca, lca,
 * rca removed, lca removed; then minority components move to a neighbouring label (> 70 % of their boundary) and
 * removed vertices are restored by round-synchronous majority votes.  Of equally large largest components the one
 * with the smallest vertex index is kept (the reference picks one of them in hash order).  A face index out of range
 * is MM_ERR_INVALID. */
int     mm_final_reclassification(const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf,
                                  const double* rca_xyz, int64_t nr, const double* lca_xyz, int64_t nl,
                                  const double* rca_removed_xyz, int64_t nrr, const double* lca_removed_xyz, int64_t nlr,
                                  uint8_t* label);

/* ---- vessel discretisation (src/ccta/discretizing).  Contours: n_points xyz triples each. ------------------------- */

#define MM_SLICE_MAX_ANCHORS     (1 << 22)   /* anchors (slices) of one branch; more is MM_ERR_INVALID   */
#define MM_DISCRETIZE_MAX_POINTS (1 << 20)   /* n_points of one resampled contour                        */

/* The number of slice anchors of branch branch_id walked every step_size (walk_centerline_slices, projecting.rs:13-60):
 * the upper bound on its contours.  0 for an absent branch or a NaN length; a step_size <= 0 or non-finite (the
 * reference never ends) or more than MM_SLICE_MAX_ANCHORS anchors is MM_ERR_INVALID. */
int64_t mm_slice_anchor_count(const mm_clpoint* cl, int64_t ncl, uint32_t branch_id, double step_size);
/* voronoi_partition + project_to_plane (:62-118) on the device, n_jobs at once.  Job j: points pt_off[j] ..
 * pt_off[j+1] (xyz triples), anchors anchor_off[j] .. anchor_off[j+1] (6 doubles each: position, unit normal).
 * anchor_idx[i] = the job-local index of point i's nearest anchor (ties: the lowest; a NaN distance to anchor 0 pins the
 * point there, a NaN distance to a later anchor never wins), proj_xyz[i] = the point projected onto that anchor's
 * plane.  A job without anchors gives -1 and the point itself. */
int     mm_nearest_anchor_project(mm_engine* e, int n_jobs, const int64_t* pt_off, const double* pts_xyz,
                                  const int64_t* anchor_off, const double* anchors, int32_t* anchor_idx, double* proj_xyz);
/* resample_spline (resampling.rs:69-90), host: the n points (in bucket order) sorted by angle about centroid, a closed
 * Catmull-Rom spline through them, n_points uniform in arc length into out.  Returns 1, or 0 where the reference
 * returns None (fewer than 3 points, no local basis, a spline shorter than 1e-10); a NaN angle (a panic in the
 * reference) or n_points outside [2, MM_DISCRETIZE_MAX_POINTS] is MM_ERR_INVALID. */
int     mm_resample_closed_contour(const double* pts, int64_t n, const double centroid[3], int64_t n_points, double* out);
/* discretize_vessel_rs (discretizing.rs:13-22) for n_jobs (centerline, branch, points) jobs in one device pass.  Job j:
 * centerline points cl_off[j] .. cl_off[j+1] of cl, branch branch_id[j], points pt_off[j] .. pt_off[j+1] (xyz).  It
 * writes n_contours[j] contours at slots out_off[j] .. : ids (the anchor index, also the original frame), centroids_xyz
 * (the anchor position) and n_points xyz triples per contour in out_xyz.  out_off[j+1] - out_off[j] must be at least
 * mm_slice_anchor_count of the job.  Same errors as mm_slice_anchor_count and mm_resample_closed_contour. */
int     mm_discretize_vessel_batch(mm_engine* e, int n_jobs, const mm_clpoint* cl, const int64_t* cl_off,
                                   const uint32_t* branch_id, const double* pts_xyz, const int64_t* pt_off,
                                   double step_size, int64_t n_points, const int64_t* out_off, int64_t* n_contours,
                                   int32_t* ids, double* centroids_xyz, double* out_xyz);

/* ---- mesh morphing (src/ccta/adjust_mesh/scale_coronary.rs:218-260, src/ccta/binding/ccta_py.rs:541-580) ---------- */

/* centerline_based_diameter_morphing (scale_coronary.rs:218-260) on the device, n_jobs at once.  Job j: centerline
 * points cl_off[j] .. cl_off[j+1] of cl, points pt_off[j] .. pt_off[j+1] (xyz), adjustment adj[j].  nearest[i] = the
 * job-local index of point i's nearest centerline point (best = DBL_MAX, index 0; a point replaces the best iff its
 * squared distance is below it: ties keep the lowest index, NaN distances never win); out_xyz[i] = p + (v / |v|) * adj
 * with v = p - that point, or p itself where |v| is 0 or NaN.  A job with points and no centerline point is
 * MM_ERR_INVALID (a panic in the reference); a job without points is fine. */
int     mm_centerline_morph_batch(mm_engine* e, int n_jobs, const mm_clpoint* cl, const int64_t* cl_off,
                                  const double* pts_xyz, const int64_t* pt_off, const double* adj, double* out_xyz,
                                  int32_t* nearest);
/* index[i] = the LAST key with the bit pattern of query i (bits_key, the reference's coord_to_idx maps), or -1.
 * Returns the number of queries matched. */
int64_t mm_match_points(const double* keys_xyz, int64_t nk, const double* queries_xyz, int64_t nq, int64_t* index);
/* keep_largest_connected_component (ccta_py.rs:541-580), host.  The points are matched to vertices by bit pattern (the
 * last of duplicated vertices wins); keep receives the vertex indices of the largest connected component of the face
 * adjacency restricted to the matched vertices, ascending (capacity n).  Of equally large ones the component holding
 * the smallest vertex index is kept (the reference picks one in hash order).  Returns their number, or 0 where the
 * reference returns the points unchanged: fewer than 2 points, or none matches a vertex.  Face indices >= nv are
 * never in the subset (as in the reference); a negative one is MM_ERR_INVALID. */
int64_t mm_keep_largest_component(const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf,
                                  const double* pts_xyz, int64_t n, int64_t* keep);

/* ---- mesh trimming (multimodars/ccta/boundary.py:26-325, stitching.py:110-352, __init__.py:341-373) --------------- */

/* Faces are nf int64 index triples into nv vertices.  A face index outside [0, nv), a negative count, or nv or nf at 2^31
 * or above is MM_ERR_INVALID (device indices are int32).  Rings follow a fixed walk rule where the reference follows
 * CPython's set order: rings are discovered in increasing order of their smallest remaining vertex and start at it; from
 * every vertex the walk goes to the smallest neighbour that is not the previous vertex and still remains; length ties
 * keep discovery order.  target_n -1 reports every ring (the reference's None); 0 or below -1 is MM_ERR_INVALID. */

/* build_adjacency_map (_processing.py:1476-1505, ccta_py.rs:507-525), host: off (nv + 1 entries) and nb (capacity 6 nf)
 * receive the sorted, de-duplicated neighbour lists in CSR form (a repeated corner makes a vertex its own neighbour). */
int     mm_build_adjacency(const int64_t* faces, int64_t nf, int64_t nv, int64_t* off, int64_t* nb);
/* The rim logic on an open-edge list (ne (a, b) pairs), host only: the rim graph (_boundary_graph), the components
 * touching the seeds (_rims_touching; every component when ns == 0), the walk, and
 *   clean == 0: _reduce_rings of the walk to target_n (order_boundary_rings);
 *   clean == 1: one round of clean_open_boundary: rim = the vertices of the rims touching the seeds (none: no rings);
 *               drop = those of degree != 2, else the _despike_ring spikes (despike_cos); else the reduced rings.
 * counts[4] = {rings, ring vertices, drop, rim}; rings go back to back into ring_idx, their lengths into ring_len; drop
 * and rim are ascending (read only with clean).  ring_len, ring_idx, drop and rim hold 2 ne entries each. */
int     mm_boundary_rings(const int64_t* edges, int64_t ne, const int64_t* seeds, int64_t ns, const double* vertices_xyz,
                          int64_t nv, int64_t target_n, double despike_cos, int clean, int64_t* ring_len,
                          int64_t* ring_idx, int64_t* drop, int64_t* rim, int64_t* counts);
/* open_boundary_edges (boundary.py:26-43) on the device: the edges used by exactly one face, as (smaller, larger) pairs
 * in lexicographic order, into edges (capacity 3 nf pairs).  Returns their number. */
int64_t mm_open_boundary_edges(mm_engine* e, const int64_t* faces, int64_t nf, int64_t nv, int64_t* edges);
/* clean_open_boundary (boundary.py:257-325): every round re-derives the faces without the dropped vertices and their
 * open edges on the device, then runs the clean round of mm_boundary_rings, growing the seeds by the rim; after
 * max_rounds the rim is ordered as it stands.  drop (capacity nv) receives the culled vertices, ascending; rings as in
 * mm_boundary_rings (capacity nv each).  counts[3] = {rings, ring vertices, drop}. */
int     mm_clean_open_boundary(mm_engine* e, const int64_t* faces, int64_t nf, const double* vertices_xyz, int64_t nv,
                               const int64_t* seeds, int64_t ns, int64_t target_n, double despike_cos,
                               int64_t max_rounds, int64_t* drop, int64_t* ring_len, int64_t* ring_idx, int64_t* counts);
/* One trim of a mesh on the device, from one upload of the mesh to one download of the result.  region[v] = 1 marks the
 * vertices of the region.
 *   mode 0 (remove_labeled_points_from_mesh, stitching.py:110-240): the vertices outside the region are kept;
 *   mode 1 (keep_labeled_points_from_mesh, :243-352): the vertices of the region are kept;
 *       both: a face survives with all three corners kept; the kept corners of the other faces seed the rim, which
 *       clean_open_boundary(target_n, despike_cos, max_rounds) cleans; the vertices it culls go too;
 *   mode 2 (_extract_region_with_border_faces, __init__.py:341-373): the faces with a corner in the region and the
 *       vertices they use.
 * out_vertices (capacity nv) and out_faces (capacity nf, remapped to the compacted order) receive the kept vertices and
 * faces in their original order; rings (modes 0 and 1; old vertex indices; capacity nv each) as in mm_boundary_rings.
 * counts[4] = {vertices, faces, rings, ring vertices}. */
int     mm_trim_mesh(mm_engine* e, const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf,
                     const uint8_t* region, int mode, int64_t target_n, double despike_cos, int64_t max_rounds,
                     double* out_vertices, int64_t* out_faces, int64_t* ring_len, int64_t* ring_idx, int64_t* counts);

/* ---- stitching (multimodars/ccta/stitching.py:69-107, 355-481, 1148-1334; _converters.py:1018-1085;
 *      src/ccta/binding/ccta_py.rs:596-700) ------------------------------------------------------------------------- */

/* What mm_mesh_assemble did and what it left.  watertight <=> n_open_edges == 0 && n_nonmanifold_edges == 0. */
typedef struct mm_assemble_report {
    int64_t n_vertices, n_faces;             /* of the result                                                        */
    int64_t n_welded_vertices;               /* referenced vertices merged into an earlier one                       */
    int64_t n_unreferenced_vertices;         /* vertices no input face names: dropped                                */
    int64_t n_degenerate_faces;              /* faces with a repeated index after the weld: dropped                  */
    int64_t n_duplicate_faces;               /* faces whose vertex set an earlier face has: dropped                  */
    int64_t n_flipped_faces;                 /* faces the winding stage reversed (not counting the inversion)        */
    int64_t n_winding_conflicts;             /* edges owned twice whose faces still disagree: 0 for orientable input */
    int64_t n_open_edges, n_nonmanifold_edges;   /* edges of the result owned by one face / by more than two         */
    int64_t inverted;                        /* 1: volume < 0 and every face was reversed                            */
    int64_t winding_rounds;                  /* launches of the winding stage's union-find: 1 hook + the pointer-    */
                                             /* jumping rounds, at most 2 + ceil(log2(max(n_faces, 2)))               */
    double  volume;                          /* signed volume before the inversion (0 without fix_inversion)         */
} mm_assemble_report;

/* fix_mesh_winding (ccta_py.rs:596-700) on the device, on a bare face list (indices in [0, 2^31), nf < 2^31).  Two
 * faces are adjacent when they share an undirected edge owned by exactly two faces.  In every connected component the
 * face with the smallest index keeps its corner order; every other face is reversed (a, b, c) -> (c, b, a) iff its
 * parity to that face is odd (adjacent faces agree when they traverse the shared edge in opposite directions).  For an
 * orientable component that is the reference's BFS whatever its hash-map order.  A component that is not orientable has
 * no consistent answer: its flips are unspecified.  info[3] = {faces reversed, edges owned twice whose faces still
 * disagree, winding_rounds}. */
int     mm_fix_winding(mm_engine* e, const int64_t* faces, int64_t nf, int64_t* out_faces, int64_t* info);
/* n_parts meshes concatenated, welded, cleaned and oriented on the device: one upload, one download.  Part p has the
 * vertices vert_off[p] .. vert_off[p+1] of vertices_xyz and the faces face_off[p] .. face_off[p+1] of faces, whose
 * indices are local to the part (checked against it before anything is allocated); the totals stay below 2^31.
 *   weld     only vertices some face names take part.  key = rint(c * 10^merge_digits) per coordinate (one f64
 *            multiply; rint rounds half to even; merge_digits in [0, 15]).  A vertex with a non-finite coordinate or a
 *            scaled magnitude at or above 2^62 matches nothing.  Vertices with equal keys become the one with the
 *            smallest index in concatenated order, coordinates bit for bit; survivors keep concatenated order.
 *   faces    remapped through the weld; a face with a repeated index is dropped; of faces with the same vertex set the
 *            one with the smallest index stays, with its own corner order; survivors keep input order.
 *   winding  (fix_winding) as mm_fix_winding on the surviving faces.
 *   inversion (fix_inversion) volume = (sum_f t_f) / 6 over the surviving faces after the winding stage, with, for the
 *            corners p0 p1 p2 of f, unfused:  cx = p1y p2z - p1z p2y;  cy = p1z p2x - p1x p2z;  cz = p1x p2y - p1y p2x;
 *            t_f = (p0x cx + p0y cy) + p0z cz.  The sum is the adjacent-pair tree over the faces in output order, padded
 *            with +0.0 to a power of two.  volume < 0: every face is reversed.
 * out_vertices (capacity: all vertices) and out_faces (capacity: all faces) receive the result. */
int     mm_mesh_assemble(mm_engine* e, int n_parts, const double* vertices_xyz, const int64_t* vert_off,
                         const int64_t* faces, const int64_t* face_off, int merge_digits, int fix_winding,
                         int fix_inversion, double* out_vertices, int64_t* out_faces, mm_assemble_report* report);

/* The seam, host only.  Rings are n xyz triples; sums run in index order; norms are sqrt((x x + y y) + z z). */

/* _assign_rings_to_ends (stitching.py:69-107): ring r = points ring_off[r] .. ring_off[r+1]; its centroid is the
 * sequential sum of its points divided by their number.  Over all ordered pairs (i, j), i != j, in loop order, the one
 * with the smallest |c_i - prox| + |c_j - dist| (strict <: the first minimum wins) goes to pair[2].  Fewer than two
 * rings or an empty ring is MM_ERR_INVALID. */
int     mm_assign_rings_to_ends(const double* rings_xyz, const int64_t* ring_off, int64_t n_rings, const double prox[3],
                                const double dist[3], int64_t pair[2]);
/* The start index of a ring: mode 0 = _rotate_to_nearest_iv (:1154-1159), the first point nearest to iv_pt; mode 1 =
 * _adjust_start_point_by_z (:1148-1151), the first point of largest z (iv_pt unused).  As numpy's argmin / argmax, the
 * first NaN wins.  n < 1 is MM_ERR_INVALID. */
int64_t mm_ring_start(const double* ring_xyz, int64_t n, int mode, const double* iv_pt);
/* 1 where the ring is to be reversed behind its first point, else 0.  mode 0 = _fix_ring_direction_by_distance
 * (:1213-1239) against every point_step-th IV point, the first n_b of them: reversed iff its summed distance is
 * strictly smaller.  mode 1 = _fix_ring_direction_by_winding (:1242-1259): the Newell normal of the IV ring
 * (_newell_normal :1194-1210; (0, 0, 1) when its length is not above 1e-10) and the ring's signed area projected on
 * it (_signed_area_projected :1176-1191): reversed iff negative. */
int     mm_ring_direction(const double* ring_xyz, int64_t n_b, const double* iv_xyz, int64_t n_iv, int mode,
                          int64_t point_step);
/* _stitch_rings (:1262-1334): the n_b + n_iv faces of the strip between a boundary ring (vertices 0 .. n_b - 1) and an
 * IV ring (n_b .. n_b + n_iv - 1) by the two-pointer walk (the boundary advances while (i+1)/n_b <= (j+1)/n_iv in
 * f64).  With outward (nullable) every face is reversed when the mean of the finite unit face normals (sequential sum
 * in face order) has a negative dot product with it.  Returns 1 where it reversed, else 0; a ring of fewer than 3
 * points is MM_ERR_INVALID. */
int     mm_stitch_rings(const double* ring_xyz, int64_t n_b, const double* iv_xyz, int64_t n_iv, const double* outward,
                        int64_t* faces);
/* The tube of geometry_to_trimesh (_converters.py:1018-1085): n_contours contours of n_points points each give
 * 2 (n_contours - 1) n_points faces [a, b, d], [b, c, d] per quad; every face is reversed when the first face's normal
 * points towards centroid0 (the first contour's centroid).  Returns 1 where it reversed; fewer than 2 contours or 1
 * point is MM_ERR_INVALID. */
int     mm_tube_faces(const double* contours_xyz, int64_t n_contours, int64_t n_points, const double centroid0[3],
                      int64_t* faces);

/* ---- rim conditioning (multimodars/ccta/stitching.py:484-1064: _prepare_prox_dist_boundary_pts and its helpers) ----- */

/* The ring arithmetic, host only, f64, unfused.  Rings are n xyz triples; a mean over points is the sequential sum in
 * index order divided by their number; dot products are (x x' + y y') + z z', norms sqrt((x x + y y) + z z).  A NULL
 * array, a negative count or a non-finite input (the reference would hand NaN on) is MM_ERR_INVALID; rings of fewer
 * than 3 points pass through where the reference passes them through. */

/* The centroid and the direction of least variance of n >= 1 points (_plane_normal_svd :965-969, :659-662): the
 * eigenvector of the smallest eigenvalue of the 3 x 3 scatter matrix by cyclic Jacobi, unit length, its component of
 * largest magnitude positive.  numpy's SVD leaves the sign open and every use in the reference is indifferent to it; the
 * direction agrees with LAPACK's to rounding only. */
int     mm_ring_fit_plane(const double* ring_xyz, int64_t n, double origin[3], double normal[3]);
/* origin == normal == NULL: _project_to_best_fit_plane (:648-665), the ring on its own plane.  Both given:
 * _project_onto_plane (:775-782), p - ((p - origin) . normal) normal. */
int     mm_ring_project_to_plane(const double* ring_xyz, int64_t n, const double* origin, const double* normal, double* out);
/* _smooth_ring_preserving_size (:706-739): `iterations` passes of alpha p_i + (1 - alpha) (p_{i-1} + p_{i+1}) / 2, then
 * scaled about the centroid back to the calibre (mean distance from the centroid) it had; a calibre of zero before or
 * after leaves the smoothed ring as it is. */
int     mm_ring_smooth_preserving_size(const double* ring_xyz, int64_t n, int64_t iterations, double alpha, double* out);
/* _redistribute_ring_evenly (:742-772): n_out points (-1: n) at the arc lengths i * (perimeter / n_out) of the closed
 * polyline; the segment of a target is the last one starting at or before it.  Index 0 keeps its bits.  n < 3, n_out < 3
 * or a zero perimeter copies the ring.  out holds max(n, n_out) points; returns the number written. */
int64_t mm_ring_redistribute(const double* ring_xyz, int64_t n, int64_t n_out, double* out);
/* _shift_plane_clear_of (:785-813): the unit normal turned along `outward`, and the plane moved along it until every
 * one of the n >= 1 points lies at least `overshoot` behind it.  *moved = the distance (0: it was clear already). */
int     mm_plane_shift_clear_of(const double origin[3], const double normal[3], const double* pts_xyz, int64_t n,
                                const double outward[3], double overshoot, double out_origin[3], double out_normal[3],
                                double* moved);
/* _clamp_to_plane (:978-1011): the side of the plane is the sign of the median distance (an even count: the mean of the
 * middle two; sign(0) = 0); a point whose distance has another sign and is not 0 goes onto the plane; with overshoot > 0
 * every point nearer than `overshoot` on the right side is then moved out to exactly that. */
int     mm_ring_clamp_to_plane(const double* ring_xyz, int64_t n, const double origin[3], const double normal[3],
                               double overshoot, double* out);
/* The insert counts of _densify_boundary (:862-892): every ring edge i (point i to point i + 1, cyclic) receives
 * (target_n - n) / n points and the (target_n - n) % n longest one more (of equal lengths the earlier edge first).
 * Returns 1 with a plan, 0 where there is nothing to insert (n < 3 or target_n == n), 2 where n > target_n (the
 * reference's warning); counts is zero then. */
int     mm_ring_densify_plan(const double* ring_xyz, int64_t n, int64_t target_n, int64_t* counts);

/* The three mesh-wide stages on the device (mm_rim_kernels.hip).  Indices on the device are int32: nv, nf < 2^31 and
 * face indices in [0, nv), checked before anything is allocated.  Every stage has one answer whatever the scheduling. */

/* The reference's {tuple(v): i} dict over the vertices (:826, :873): index[k] = the LAST vertex equal to point k by
 * value (-0.0 equals 0.0, a row with a NaN equals nothing), -1 without one. */
int     mm_mesh_locate_points(mm_engine* e, const double* vertices_xyz, int64_t nv, const double* pts_xyz, int64_t r,
                              int64_t* index);
/* Query points one LDS chunk of that kernel holds (more are staged chunk after chunk). */
int     mm_rim_locate_chunk_points(void);
/* _enforce_layer_gap_from_plane (:1014-1064).  out_layer[v] = 0 for a seed, k for a vertex whose shortest path to a
 * seed over face edges has k <= n_rings edges, else -1.  A vertex p of layer k >= 1 moves, unfused and in this order:
 *   d = ((px - ox) nx + (py - oy) ny) + (pz - oz) nz;  q = p - d n;  r = q - o;  rn = sqrt((rx rx + ry ry) + rz rz);
 *   rn < 1e-10: it stays;  else p + ((k step) / rn) r.
 * One launch marks the seeds, one finds each ring (the run ends behind a ring that finds no vertex), one pushes.
 * info[3] = {kernel launches, rings run, vertices with a layer >= 1}. */
int     mm_mesh_layer_push(mm_engine* e, const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf,
                           const int64_t* seeds, int64_t ns, const double origin[3], const double normal[3],
                           double layer_step, int64_t n_rings, double* out_vertices, int32_t* out_layer, int64_t* info);
/* The mesh side of _densify_boundary (:894-962) for a ring of n >= 3 distinct vertices (a repeated one is
 * MM_ERR_INVALID; the reference would overwrite its own table) and counts[i] points for ring edge i.
 *   vertices  the input vertices; then, edge after edge, the points pa + (j / (count + 1)) (pb - pa), j = 1 .. count;
 *             then one centroid (the mean of the polygon's points) per face fanned about a centroid, in face order.
 *   faces     a face is touched when one of its edges joins the two ends of a ring edge with count > 0, in either
 *             direction.  The untouched faces come first, in input order.  Then, in ascending order of the touched
 *             face, its fan: the face's polygon is its corners in order with the inserted points of each edge behind
 *             the edge's first corner; about the first corner that is on no subdivided edge, (r0, r_i, r_i+1) over the
 *             polygon rotated to start there; without such a corner about the centroid, (c, p_i, p_i+1) all round.
 *             (The reference walks a Python set of touched faces: its order is CPython's.)
 *   ring      out_ring_idx (n + sum(counts) entries): every ring vertex followed by its edge's inserted points.
 * info[6] = {vertices, faces, points inserted, faces fanned, fans about a centroid, kernel launches}.  Where vert_cap
 * or face_cap is too small nothing else is written, info[0..1] hold the sizes needed, and the call returns
 * MM_ERR_TOO_LARGE. */
int     mm_mesh_split_rim_edges(mm_engine* e, const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf,
                                const int64_t* ring_idx, int64_t n, const int64_t* counts, int64_t vert_cap,
                                int64_t face_cap, double* out_vertices, int64_t* out_faces, int64_t* out_ring_idx,
                                int64_t* info);

typedef struct mm_rim_params {
    int64_t proximal_is_ostium;              /* != 0: _condition_ostium_ring on the proximal ring                      */
    int64_t target_n;                        /* points of a densified ring; 0: no densification (the reference's None) */
    int64_t smooth_iterations, n_rings;      /* the reference's 5 and 2                                                */
    int64_t vert_cap, face_cap, ring_cap;    /* capacities of out_vertices, out_faces and of each ring                 */
    double  smooth_alpha;                    /* 0.5                                                                    */
    double  angle_threshold_deg;             /* 45                                                                     */
    double  clamp_overshoot;                 /* mm                                                                     */
    double  layer_step_mm;                   /* 0.1                                                                    */
} mm_rim_params;

/* What mm_condition_rims did.  The reference's printed warnings are the ring_* flags. */
typedef struct mm_rim_report {
    int64_t n_vertices, n_faces;             /* of the result                                                          */
    int64_t n_prox, n_dist;                  /* points of the returned rings                                           */
    int64_t n_moved_prox, n_moved_dist;      /* mesh vertices the first write-back of each ring moved                  */
    int64_t n_moved_ostium;                  /* ... and the write-back of the ostium stage                             */
    int64_t clamped;                         /* 1: the planes met at the threshold angle or above, the clamp ran       */
    int64_t n_layer_vertices[2];             /* vertices of layer 1 and 2 behind a clamped ring                        */
    int64_t n_inserted_prox, n_inserted_dist;
    int64_t n_fanned_faces, n_centroid_fans; /* faces replaced by a fan; those of them fanned about a centroid         */
    int64_t ring_over_target[2];             /* the ring has more points than target_n: left as it is                  */
    int64_t ring_off_mesh[2];                /* a point of the ring is no mesh vertex: not densified                   */
    int64_t n_launches;                      /* kernels launched                                                       */
    int64_t bytes_uploaded, bytes_downloaded;/* all copies of the call: the mesh once each way, the rest ring-sized    */
    double  plane_shift_mm;                  /* how far the ostium plane moved (0: it was clear, or no ostium stage)   */
    double  plane_angle_deg;                 /* the angle between ring plane and IV plane (0 without the ostium stage) */
} mm_rim_report;

/* _prepare_prox_dist_boundary_pts (:505-556) for the two rings already assigned to the ends: one upload of the mesh, one
 * download, the mesh resident in between.  Both rings: project, smooth, redistribute, written back to the vertices they
 * are located at (a ring that gives one vertex two different targets is MM_ERR_INVALID; the reference keeps the last).
 * With proximal_is_ostium, n_iv > 0 and n_prox >= 3 the ostium stage (:582-645): towards = the mean of aorta_xyz minus
 * the ring's centroid, or prox_outward (nullable) where that is zero or na == 0; the plane shift, the clamp against the
 * IV plane through prox_centroid where the angle reaches the threshold, the write-back, and behind a clamped ring the
 * layer push of mm_mesh_layer_push from the moved vertices.  Then, with target_n > 0, both rings densified
 * (mm_ring_densify_plan, mm_mesh_locate_points, mm_mesh_split_rim_edges), proximal first.
 * Launches: 1 to locate a ring, 1 to write it (none where no point sits on the mesh); 1 + rings run + 1 for the layer
 * push; to split, 3 (positions, ring coordinates, touched faces) and 4 more (scan, compaction) where a face is touched.
 * Capacities as mm_fill_holes: too small, the call returns MM_ERR_TOO_LARGE and n_vertices / n_faces of the report hold
 * sizes that suffice for a rim whose edges have one owner each (n_prox / n_dist the ring sizes). */
int     mm_condition_rims(mm_engine* e, const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf,
                          const double* prox_ring, int64_t n_prox, const double* dist_ring, int64_t n_dist,
                          const double* iv_frame, int64_t n_iv, const double prox_centroid[3], const double* prox_outward,
                          const double* aorta_xyz, int64_t na, const mm_rim_params* params, double* out_vertices,
                          int64_t* out_faces, double* out_prox, double* out_dist, mm_rim_report* report);

/* ---- mesh closing (multimodars/ccta/fixing_functions.py:13-49, multimodars/ccta/__init__.py:432-499;
 *      src/ccta/binding/ccta_py.rs:743-814) ------------------------------------------------------------------------- */

/* What mm_fill_holes did and what it left.  watertight <=> n_open_edges == 0 && n_nonmanifold_edges == 0. */
typedef struct mm_fill_report {
    int64_t n_vertices, n_faces;             /* of the result: nv + n_loops_filled, nf + n_fan_faces                 */
    int64_t n_loops_filled, n_fan_faces;     /* loops of at least 3 vertices, and the faces of their fans            */
    int64_t n_open_edges_before;             /* open edges of the input (after the winding stage)                    */
    int64_t n_short_loops;                   /* loops of fewer than 3 vertices: skipped, their edges stay open       */
    int64_t n_irregular_components;          /* rim components with a vertex that is not regular: left open          */
    int64_t n_irregular_edges;               /* the open edges they hold                                             */
    int64_t n_open_edges, n_nonmanifold_edges;   /* edges of the result owned by one face / by more than two         */
    int64_t n_flipped_faces;                 /* faces the winding stage reversed (not counting the inversion)        */
    int64_t winding_rounds;                  /* as mm_assemble_report: at most 2 + ceil(log2(max(nf, 2)))            */
    int64_t inverted;                        /* 1: volume < 0 and every face of the result was reversed              */
    double  volume;                          /* signed volume of the result before the inversion (0 without          */
                                             /* fix_normals)                                                         */
} mm_fill_report;

/* The walk over the rim, host only (no engine, no device).  half_edges: ne (a, b) pairs, the open edges as their owner
 * traverses them, in any order; indices in [0, nv).  succ(a) = b.  A vertex is regular iff exactly one half-edge leaves
 * it and exactly one enters it.  The half-edges fall into components (two half-edges with a common vertex belong
 * together).  A component all of whose vertices are regular is one cycle of succ: a loop.  Loops are reported in
 * increasing order of their smallest vertex, start at it and follow succ; a loop of fewer than 3 vertices
 * (fixing_functions.py:27) is counted and skipped.  Every other component is irregular (a pinch vertex, faces that
 * disagree in direction along the rim, a non-manifold edge nearby): counted and skipped.  Loop k's centroid is the sum
 * of its points in walk order, per coordinate, sequential, divided by their number (f64, unfused).
 * loop_len (capacity ne), loop_idx (capacity ne) and centroids (capacity ne doubles: 3 per loop; nullable, as is
 * vertices_xyz then) receive the loops back to back.  counts[5] = {loops, loop vertices, irregular components,
 * irregular edges, short loops}. */
int     mm_hole_loops(const int64_t* half_edges, int64_t ne, const double* vertices_xyz, int64_t nv, int64_t* loop_len,
                      int64_t* loop_idx, double* centroids, int64_t* counts);
/* manual_hole_fill (fixing_functions.py:13-49): every regular loop of the open rim closed by a fan about its centroid.
 * One upload of the mesh, one download of the result; everything proportional to nf runs on the device
 * (mm_weld_kernels.hip, mm_close_kernels.hip), the walk of mm_hole_loops on the host.  nv, nf < 2^31 and face indices
 * in [0, nv), checked before anything is allocated.
 *   winding   (fix_normals != 0) the faces first go through the winding stage exactly as mm_fix_winding defines it.
 *   open half-edges  an undirected edge owned by exactly one face is open; its owner traverses it a -> b.
 *   loops     as mm_hole_loops on the open half-edges.
 *   fill      loop k (of at least 3 vertices) gets the new vertex nv + k, its centroid.  For each half-edge a -> b of
 *             the loop, in walk order, the face (b, a, nv + k) is appended: it crosses the shared edge against the
 *             owner, so the fan agrees with the mesh around it.  New faces follow all input faces, loop after loop;
 *             input vertices keep their index and their bits.
 *   orientation  (fix_normals != 0) the inversion stage of mm_mesh_assemble on the result: the same t_f, the same
 *             adjacent-pair tree over the faces of the result in output order, volume < 0 reverses every face.
 * Bounds: loops <= open edges / 3, fan faces <= open edges <= 3 nf.  When vert_cap < nv + loops or face_cap < nf + fan
 * faces, nothing but the report is written and the call returns MM_ERR_TOO_LARGE; n_vertices and n_faces of the report
 * then hold the capacities needed (the counts found so far are filled in, those of the result are 0). */
int     mm_fill_holes(mm_engine* e, const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf,
                      int fix_normals, int64_t vert_cap, int64_t face_cap, double* out_vertices, int64_t* out_faces,
                      mm_fill_report* report);
/* smooth_mesh_labels (ccta_py.rs:743-814) on the device.  One iteration reads the labels of the previous one only.  A
 * vertex with at least one neighbour, all of whose neighbours carry the same label L != its own, becomes L; everything
 * else stays.  Only unanimous votes flip, so the result is exact and free of any order.  An iteration that flips
 * nothing ends the run.  The labels stay on the device across iterations: one upload, one download, at most two
 * launches per iteration.  info[4] = {iterations run, flips in total, flips of the last iteration run, kernel launches}.
 * A flip count above zero is no sign of progress: two vertices that are each other's only neighbour swap for ever.
 *   _faces  the neighbours of a vertex are those of mm_build_adjacency: every other corner of every face that names it,
 *           and itself where a face repeats a corner.  Face indices in [0, nv).
 *   _csr    the neighbours of vertex i are nb[off[i] .. off[i + 1]) as given (off: nv + 1 ascending entries from 0; the
 *           lists need not be symmetric, sorted or free of repeats).  A neighbour outside [0, nv) is MM_ERR_INVALID.
 * nv, nf and off[nv] stay below 2^31; iterations < 0 is MM_ERR_INVALID; on an error out_labels is not written. */
int     mm_smooth_labels_faces(mm_engine* e, const uint8_t* labels, int64_t nv, const int64_t* faces, int64_t nf,
                               int64_t iterations, uint8_t* out_labels, int64_t* info);
int     mm_smooth_labels_csr(mm_engine* e, const uint8_t* labels, int64_t nv, const int64_t* off, const int64_t* nb,
                             int64_t iterations, uint8_t* out_labels, int64_t* info);

/* ---- mesh smoothing (multimodars/ccta/fixing_functions.py:52-92: the filter_taubin that ends the post-processing;
 *      trimesh.smoothing.filter_taubin / filter_laplacian with equal weights; the isotropic remesh in front of it is not
 *      part of this project) ----------------------------------------------------------------------------------------
 *
 * Adjacency.  The neighbours of vertex v are the distinct vertices w != v that share a corner pair with v in some face.
 * A face (a, a, b) gives only a-b; repeated faces add nothing.  Row v lists its neighbours in ascending index order;
 * deg(v) is the row's length, and a vertex with deg == 0 is isolated.  (Not mm_build_adjacency, which keeps self entries
 * and no order.)
 *
 * One step with factor f.  All arithmetic is f64 and unfused.  Per coordinate x of a vertex v with deg > 0:
 *     w = 1.0 / deg;  acc = +0.0;  for the neighbours j ascending: acc = acc + w * x_j  (the product rounded, then the
 *     sum);  d = acc - x;  x' = x + f * d.
 * Every step reads the coordinates of the step before only.  Isolated and pinned vertices keep their bits; pinned
 * vertices still feed their neighbours' averages.  Non-finite coordinates propagate by IEEE.
 *
 * Schedules.  filter_taubin(lamb, nu, iterations) is the factors lamb, -nu, lamb, -nu, ... (step 0 takes lamb; x - nu d
 * and x + (-nu) d are the same bits); filter_laplacian(lamb, iterations) is lamb every step.  The C ABI takes the
 * factor array itself.
 *
 * trimesh.  This is trimesh's operator (laplacian_calculation with equal weights, L V - V) with the row order fixed;
 * trimesh's own row order follows a graph library's insertion order, so parity with it holds up to the order of the sum
 * only.  trimesh pulls an unreferenced vertex towards the origin (an empty row makes L v = 0); here it stays, counted.
 *
 * Ring distance.  ring[v] = the fewest edges of the adjacency from v to any seed vertex, 0 at a seed; -1 where that is
 * more than max_ring or no seed is reachable.
 *
 * Report.  volume_before / volume_after: the signed volume of mm_mesh_assemble (the same t_f, the same adjacent-pair
 * tree over the faces in input order, divided by 6) on the input and the output coordinates.  max_displacement_sq: the
 * largest (dx dx + dy dy) + dz dz over the vertices, d = output - input; unspecified where a coordinate is not finite.
 *
 * Device indices are int32: nv, nf < 2^31 and face indices in [0, nv), checked before anything is allocated
 * (MM_ERR_INVALID); the rows hold at most 6 nf entries, which must stay below 2^31 as well (MM_ERR_TOO_LARGE).
 * Launches.  The adjacency is 7 kernels: the edge table of mm_mesh_assemble (1), the degrees (1), their exclusive scan
 * (3), the fill (1), the sort inside each row (1).  A volume is 1 + max(1, ceil(ceil(log2 nf) / 8)).  With nv == 0 or
 * nf == 0 nothing is launched: every vertex is isolated, the volumes are 0. */

typedef struct mm_smooth_report {
    int64_t n_vertices, n_faces, n_edges;    /* n_edges: distinct undirected edges between distinct vertices          */
    int64_t n_isolated, n_pinned, max_degree;/* n_pinned: nonzero entries of the mask                                 */
    int64_t steps_run, launches;             /* launches: adjacency + n_steps + two volumes + 1 (the displacement)    */
    double  volume_before, volume_after, max_displacement_sq;
} mm_smooth_report;

/* The adjacency as CSR.  off: nv + 1 entries; nb: capacity nb_cap (6 nf always suffices).  info[4] = {entries, longest
 * row, isolated vertices, kernel launches}.  Where nb_cap is too small, info is filled (info[0] = the capacity needed),
 * off and nb are not written and the call returns MM_ERR_TOO_LARGE. */
int     mm_mesh_adjacency_csr(mm_engine* e, const int64_t* faces, int64_t nf, int64_t nv, int64_t nb_cap, int64_t* off,
                              int64_t* nb, int64_t* info);
/* n_steps steps with factors[0 .. n_steps) on the device (mm_smooth_kernels.hip): one upload of vertices, faces and mask,
 * the coordinates resident in two buffers in between, one download of the vertices and the report's numbers.  pinned
 * (nullable): nv bytes, nonzero = the vertex does not move.  n_steps == 0 copies the input bit for bit, with the report
 * filled and the volumes equal; n_steps < 0 is MM_ERR_INVALID.  out_vertices may be vertices_xyz. */
int     mm_mesh_smooth(mm_engine* e, const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf,
                       const double* factors, int64_t n_steps, const uint8_t* pinned, double* out_vertices,
                       mm_smooth_report* report);
/* ring_out[v] (nv entries) = the ring distance from the n_seeds seeds, cut at max_ring: one launch marks the seeds, one
 * finds each ring; the run stops at max_ring or behind a ring that reaches nothing.  info[3] = {vertices with a ring
 * >= 0, ring launches run, kernel launches}.  max_ring < 0 or a seed outside [0, nv) is MM_ERR_INVALID. */
int     mm_mesh_vertex_rings(mm_engine* e, const int64_t* faces, int64_t nf, int64_t nv, const int64_t* seeds,
                             int64_t n_seeds, int64_t max_ring, int32_t* ring_out, int64_t* info);

/* ---- mesh refinement (multimodars/ccta/fixing_functions.py:114-239: fix_and_remesh_stitched_mesh brings the coarse CCTA
 *      triangles down to the intravascular resolution with MeshLab's isotropic remesh; of that filter this is the edge
 *      split alone; the flip is "mesh edge flips", the tangential relaxation and the reprojection "mesh relaxation" below;
 *      the collapse is "mesh edge collapse", the repair "mesh repair") ---------------------------------------------------------------------------------------
 *
 * One pass on vertices v (f64) and triangles, with thr2 = (ratio target_len) (ratio target_len) computed once in f64:
 *   marked     the undirected edge lo < hi is marked when ((dx dx + dy dy) + dz dz) > thr2, d = v[hi] - v[lo] per
 *              component, unfused f64.  An (a, a) edge is never marked; a NaN length marks nothing.
 *   numbering  marked edges are numbered in order of first appearance: the faces ascending, in each the corners j = 0, 1,
 *              2 for the edges (c0, c1), (c1, c2), (c2, c0).  The k-th marked edge gets vertex nv + k, its coordinates
 *              (v[lo] + v[hi]) * 0.5 per component, its parents (lo, hi).
 *   children   every face (a, b, c) is replaced, in place and in face order, by children of its winding; m0, m1, m2 are
 *              the midpoints of (a, b), (b, c), (c, a).
 *                none marked   the face itself
 *                one           rotated so that the marked edge is (a, b): (a, m0, c), (m0, b, c)
 *                two           rotated so that the unmarked edge is (c, a): (m0, b, m1), then the quad a, m0, m1, c cut by
 *                              its shorter diagonal: |m0 - c|^2 < |a - m1|^2 (the squared length above, on the stored
 *                              midpoints) gives (a, m0, c), (m0, m1, c); otherwise, ties included, (a, m0, m1), (a, m1, c)
 *                three         (a, m0, m2), (m0, b, m1), (m2, m1, c), (m0, m1, m2)
 * The rule is per edge, so every owner of an edge sees the same midpoint: a third owner of a non-manifold edge, both
 * corners of a degenerate (a, b, a) face.  No existing vertex moves or changes its index.  Passes repeat on the result
 * until one marks nothing (converged), max_passes have run, or one would bring the vertices above max_vertices: that
 * pass is not run (stopped_by_cap) and the result of the passes before it is returned.
 *
 * Edges of the report: n_edges counts the distinct undirected edges between different vertices, longest_sq is the largest
 * squared length among them that is not NaN; an edge (an (a, a) edge too) with one owning corner is open, with more than
 * two non-manifold, as mm_fill_holes counts them.  The volumes are those of mm_mesh_assemble (the same t_f, the same
 * adjacent-pair tree over the faces in their order, divided by 6).
 *
 * Device indices are int32: nv, nf < 2^31 and indices in [0, nv) (MM_ERR_INVALID), 6 nf < 2^31 for the input and for
 * every pass's result, and a result below 2^31 vertices (MM_ERR_TOO_LARGE).  The mesh is uploaded once, stays on the
 * device in two buffers that take turns and grow there, and comes down once together with the parents; each pass reads
 * 80 bytes of counters back.  bytes_uploaded = 24 nv + 12 nf; bytes_downloaded = 24 nv' + 12 nf' + 8 (nv' - nv).
 * Launches (mm_refine_kernels.hip; all integer atomics, no float atomics): a pass that splits is 6 -- the edge table
 * with each edge's first corner (1), the marks and the edge counts (1), the children and new vertices per face with
 * their tile sums (1), the scan of the tile sums (1), the offsets with the midpoints and parents (1), the children (1).
 * A pass that marks nothing or is stopped by max_vertices ends behind the scan: 4.  Where max_passes passes have run,
 * the edge counts of the result cost 2 more.  The two volumes: 1 + max(1, ceil(ceil(log2 nf) / 8)) each.  With nv == 0
 * or nf == 0 nothing is launched and the input is returned. */

#define MM_REFINE_SPLIT_SLOTS 16

typedef struct mm_refine_report {
    int64_t n_vertices, n_faces;             /* of the result (the capacities needed where they were too small)       */
    int64_t n_edges_before, n_edges_after;
    int64_t passes_run;                      /* passes whose marks were taken: the last may have marked nothing       */
    int64_t splits_per_pass[MM_REFINE_SPLIT_SLOTS];   /* marked edges of pass k; passes beyond 16 add into the last   */
    int64_t faces_by_template[4];            /* faces of all passes run, by their number of marked corners            */
    int64_t converged;                       /* 1: the last pass run marked nothing                                   */
    int64_t stopped_by_cap;                  /* 1: the next pass would have passed max_vertices and was not run       */
    int64_t n_open_edges_before, n_open_edges_after;
    int64_t n_nonmanifold_edges_before, n_nonmanifold_edges_after;
    int64_t n_launches, bytes_uploaded, bytes_downloaded;
    double  longest_sq_before, longest_sq_after;
    double  volume_before, volume_after;
} mm_refine_report;

/* The first half of a pass made public: the distinct undirected edges between different vertices in order of first
 * appearance (out_edges: lo, hi per edge) with their squared lengths as the marking computes them.  info[4] = {edges,
 * open edges, non-manifold edges, kernel launches (the 4 of a stopped pass, 1 more for the list)}.  Where edge_cap is
 * too small, info is filled (the list was not launched), nothing else is written and the call returns MM_ERR_TOO_LARGE. */
int     mm_mesh_edge_lengths(mm_engine* e, const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf,
                             int64_t edge_cap, int64_t* out_edges, double* out_len_sq, int64_t* info);
/* The passes above.  target_len and ratio finite and > 0, with a threshold that neither overflows nor underflows to 0;
 * max_passes >= 0 (0 returns the input, with the edge counts and volumes of the report filled); max_vertices >= 0.
 * out_vertices: vert_cap triples, out_tris: face_cap triples, out_parents: 2 per new vertex, capacity vert_cap - nv
 * pairs.  Capacities as mm_fill_holes: where vert_cap or face_cap is too small, nothing but the report is written (all of
 * it: n_vertices and n_faces are the capacities needed) and the call returns MM_ERR_TOO_LARGE.  On any other error the
 * outputs are not written. */
int     mm_mesh_refine(mm_engine* e, const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf,
                       double target_len, double ratio, int64_t max_passes, int64_t max_vertices, int64_t vert_cap,
                       int64_t face_cap, double* out_vertices, int64_t* out_tris, int64_t* out_parents,
                       mm_refine_report* report);

/* ---- surface distance ---------------------------------------------------------------------------------------------
 * How far a point lies from a triangle mesh: the quantity the reference bounds inside MeshLab while it remeshes
 * (multimodars/ccta/fixing_functions.py:196-219, checksurfdist / maxsurfdist) and this project measures instead.
 * tests/mm_checkers/surface_distance.py is the executable form of the rule.
 *
 * For a query p and a face (a, b, c), all arithmetic unfused f64, dot(u, v) = (ux*vx + uy*vy) + uz*vz, u + e*t one
 * product and one sum per component, every quotient a true IEEE division.
 *
 * Proper faces take Ericson's closest point (Real-Time Collision Detection 5.1.5); the first test that holds wins:
 *   1. ab = b-a, ac = c-a, ap = p-a; d1 = dot(ab,ap), d2 = dot(ac,ap).  d1 <= 0 && d2 <= 0: a (region 1).
 *   2. bp = p-b; d3 = dot(ab,bp), d4 = dot(ac,bp).  d3 >= 0 && d4 <= d3: b (region 2).
 *   3. vc = d1*d4 - d3*d2.  vc <= 0 && d1 >= 0 && d3 <= 0: a + ab*(d1/(d1-d3)) (edge ab, region 4).
 *   4. cp = p-c; d5 = dot(ab,cp), d6 = dot(ac,cp).  d6 >= 0 && d5 <= d6: c (region 3).
 *   5. vb = d5*d2 - d1*d6.  vb <= 0 && d2 >= 0 && d6 <= 0: a + ac*(d2/(d2-d6)) (edge ca, region 6).
 *   6. va = d3*d6 - d5*d4.  va <= 0 && (d4-d3) >= 0 && (d5-d6) >= 0: b + (c-b)*((d4-d3)/((d4-d3)+(d5-d6))) (edge bc,
 *      region 5).
 *   7. otherwise s = (va+vb)+vc and the point is (a + ab*(vb/s)) + ac*(vc/s) (interior, region 0).
 * d2(p, face) = dot(p-q, p-q) for the closest point q.
 *
 * Degenerate faces -- a repeated index, or every component of ab x ac = (aby*acz - abz*acy, abz*acx - abx*acz,
 * abx*acy - aby*acx) exactly 0.0 -- take the smallest d2 over the segments ab, bc, ca in that order with strict <.  For a
 * segment (u, v): e = v-u; l = dot(e,e); t = 0 where l == 0, else dot(p-u,e)/l, replaced by 0 where it is < 0 and by 1
 * where it is > 1; the point is u + e*t.  The region is 4, 5 or 6 for the winning segment.
 *
 * Thin faces -- not degenerate, and dot(n, n) < 2^-34 * (l*l) with n = ab x ac as above and l the largest of dot(ab,ab),
 * dot(ac,ac), dot(bc,bc), bc = c-b: the smallest altitude is below 2^-17 of the longest edge, as computed -- do not go
 * through the tests 1 to 7, whose cross terms va, vb, vc are cancellation noise on such a face.  They take the segment
 * rule of the degenerate faces first; then, with d1 .. d6, vc, vb, va as in 1 to 6, where va > 0 && vb > 0 && vc > 0, the
 * interior point of 7 replaces the segments' point iff its d2 is strictly smaller (region 0).  Every candidate is a convex
 * combination of the corners up to rounding, so the closest point is a point of the closed triangle and d2 is never too
 * small; the nearest segment point is within the inradius (at most half the smallest altitude) of the true closest point,
 * so the distance is too large by at most that.  A face that is neither degenerate nor thin is proper.
 *
 * The fold over faces is exact: face f replaces the best iff its d2 < best, so equal d2 keeps the lowest face index and a
 * NaN d2 is never chosen; a query that no face beat returns +inf, face -1, closest NaN, region -1.  The result has one
 * bit pattern whatever the chunking, the order or the pruning.  The device computes every d2 (mm_tri_kernels.hip). */

typedef struct mm_surface_report {
    int64_t items_pass_a;     /* (query block, face chunk) items that always run: one per query block */
    int64_t items_pass_b;     /* the others, which first check their lower bound against the block's minima */
    int64_t items_skipped;    /* those of pass B that the check skipped */
    int64_t n_launches;
    int64_t bytes_uploaded, bytes_downloaded;
} mm_surface_report;

/* out_sq[i] = the smallest d2 of query i over the nf faces; out_face (nullable) the winning face, out_closest (nullable,
 * 3 per query) its closest point, out_region (nullable) the region.  nf == 0 or nq == 0 is valid.  MM_ERR_INVALID: a
 * non-finite coordinate in vertices or queries, a face index out of range, nv, nf or nq of 2^31 or more; MM_ERR_TOO_LARGE:
 * more than 2^31 - 1 (query block, chunk) items.  On an error the outputs are not written. */
int     mm_point_mesh_distance(mm_engine* e, const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf,
                               const double* queries_xyz, int64_t nq, double* out_sq, int64_t* out_face,
                               double* out_closest, int32_t* out_region, mm_surface_report* report);
/* TEST HOOK (nothing in the product calls it; no engine, no device): the host side of mm_point_mesh_distance.
 * face_order[j] = the face staged at position j, query_perm[j] = the query staged at position j (slabs across the longest
 * axis of the faces' corners, faces by the sum of their corners: ascending up to one cell of a 20-bit quantisation of
 * the range).  items (3 int32 each: 0 = pass A, 1 = pass B; first staged query q0; first staged face c0) and item_lb2 (the item's lower bound of every d2 between its queries and its
 * faces) receive at most cap items, pass A first.  info[4] = {items of pass A, of pass B, queries per block, faces per
 * chunk}.  Errors as mm_point_mesh_distance. */
int     mm_tri_plan(const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf, const double* queries_xyz,
                    int64_t nq, int32_t* face_order, int32_t* query_perm, int64_t* info, int32_t* items, double* item_lb2,
                    int64_t cap);

/* ---- mesh relaxation (multimodars/ccta/fixing_functions.py:192-219: of MeshLab's isotropic remesh the tangential
 *      smoothing and the reprojection, smoothflag / reprojectflag / checksurfdist; the flip is "mesh edge flips" below,
 *      the collapse is "mesh edge collapse", the repair "mesh repair") ----------------------------------------------------------
 * Slides the free vertices of a mesh (v, faces) along a reference surface (rv, rfaces; the mesh's own input where none is
 * given) and puts every one of them back on it exactly.  tests/mm_checkers/relax_mesh.py is the executable form.  All
 * arithmetic is unfused f64 in the order written; dot, the cross components and the closest point are those of "surface
 * distance", the average is that of "mesh smoothing".
 *
 * Free.  A vertex is free iff it has a neighbour in the adjacency of mm_mesh_adjacency_csr, its mask byte is 0 (or there
 * is no mask), and it ends no edge whose owner count is not 2 -- every corner pair of every face owns its undirected
 * edge, an (a, a) pair too, as mm_fill_holes and mm_mesh_refine count.  The ends of such edges are the border vertices
 * (n_border, whatever their mask byte).  A vertex that is not free keeps its input bits and still feeds its neighbours'
 * averages.  A free vertex with ref_nf == 0 is MM_ERR_INVALID.
 *
 * Projection.  P(p), F(p), D(p): closest point, winning face and d2 of the surface distance on the reference -- the
 * lowest face on ties, a degenerate face as its segments.  Where no face beats +inf (F = -1) the vertex is not moved,
 * then or later.
 *
 * Step 0 (always, n_iterations == 0 too).  For every free v:  x_v = P(v_in), F_v = F(v_in);  initial_distance_sq is the
 * largest D(v_in).
 *
 * One iteration, reading only the state before it.  For a free v with neighbours j ascending:
 *     w = 1.0 / deg;  acc = +0.0;  acc = acc + w * x_j;  d = acc - x   (per component)
 *     n = ab x ac of reference face F_v = (aby*acz - abz*acy, abz*acx - abx*acz, abx*acy - aby*acx);  nn = dot(n, n)
 *     nn > 0 and finite:  s = dot(n, d) / nn;  t = d - n*s  (one product, one difference);  otherwise t = d
 *     c = x + lambda*t  (product, then sum).  A c with a non-finite component is not used: the vertex stays and counts
 *     as reverted.  Otherwise  x'_v = P(c), F'_v = F(c);  F(c) == -1 reverts as well.
 * Guard, one round an iteration, not cascading.  For every mesh face (i, j, k) of three distinct indices:
 *     m_old = (x_j - x_i) x (x_k - x_i),  m_new the same on x';  where dot(m_old, m_old) > 0 and not
 *     dot(m_old, m_new) > 0, the face's free corners take back x and F.
 * n_reverted sums the vertices reverted over the iterations (each once an iteration).  n_flipped_faces counts the faces
 * of three distinct indices with dot(m_in, m_in) > 0 and dot(m_in, m_out) <= 0, m_in on the input, m_out on the output:
 * one guard round promises no flip-free result.
 *
 * The minimum over faces is exact, so the result has one bit pattern whatever the chunking, the order or the pruning.
 *
 * Device.  One upload: the faces (int32), the input vertices and, where a vertex is free, the reference's staged faces
 * (96 bytes each, slab order), the free vertices' input positions as queries in slab order (24), their vertex indices
 * (4), the (query block, chunk) items (16) and the chunks' boxes (48).  The mask is used on the host only.  One download:
 * the vertices, one key per query, 256 bytes of numbers.  Every buffer is rounded up to 256 bytes.  Nothing crosses in
 * between: per iteration the device recomputes each query block's box from the candidates and every item's lower bound
 * from it with the functions the host used (mm_prune.h: box_lb2, tri_slack), seeds each query's minimum with the d2 to
 * its previous face and runs every item checked.  items_run + items_skipped = items * (1 + n_iterations);
 * items_skipped - items_skipped_step0 are the skips of the iterations, on the refreshed bounds.
 * Launches, with T = 4 + (more than one chunk), V = 1 + max(1, ceil(ceil(log2 nf) / 8)), I = n_iterations:
 *     n_launches = 2 V + 2  +  [n_free > 0] (T + 1 + 6 I)  +  [n_free > 0 and I > 0] 7
 * -- two volumes, the flipped faces, the displacement; step 0 and its acceptance; per iteration the candidates with
 * seeds and bounds, the checked minima, the winners, the closest points, the guard, the acceptance; the adjacency.  With
 * nv == 0 or nf == 0 nothing is launched, the input is returned and the volumes are 0.
 *
 * Limits as mm_point_mesh_distance for both meshes (sizes below 2^31, finite coordinates, indices in range:
 * MM_ERR_INVALID; more than 2^31 - 1 items: MM_ERR_TOO_LARGE), 6 nf < 2^31 (MM_ERR_TOO_LARGE); n_iterations < 0 or a
 * non-finite lambda: MM_ERR_INVALID.  On an error no output is written. */

typedef struct mm_relax_report {
    int64_t n_vertices, n_faces, n_ref_faces;
    int64_t n_free, n_pinned, n_border, n_isolated;   /* n_pinned: nonzero mask bytes; n_isolated: no neighbour        */
    int64_t iterations_run, n_reverted, n_flipped_faces;
    int64_t items_run, items_skipped;                 /* (query block, chunk) items of the minima passes               */
    int64_t items_skipped_step0;                      /* those of items_skipped that step 0 skipped, on the host's bounds */
    int64_t n_launches, bytes_uploaded, bytes_downloaded;
    double  initial_distance_sq, max_displacement_sq; /* the latter as mm_smooth_report                                */
    double  volume_before, volume_after;              /* as mm_smooth_report                                           */
} mm_relax_report;                                    /* 160 bytes */

/* ref_vertices == NULL: the mesh itself is the reference (ref_nv, ref_tris, ref_nf are ignored).  pinned (nullable): nv
 * bytes.  out_vertices: nv triples (may be vertices_xyz); out_ref_face: nv entries, the reference face each free vertex
 * lies on, -1 where the vertex is not free. */
int     mm_mesh_relax(mm_engine* e, const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf,
                      const double* ref_vertices, int64_t ref_nv, const int64_t* ref_tris, int64_t ref_nf,
                      const uint8_t* pinned, int64_t n_iterations, double factor, double* out_vertices,
                      int64_t* out_ref_face, mm_relax_report* report);

/* ---- mesh edge flips (multimodars/ccta/fixing_functions.py:207-219: of MeshLab's isotropic remesh the swap, swapflag;
 *      the collapse is "mesh edge collapse" below) ----------------------------------------------------------------------
 * Flips edges of a mesh (v, faces) until no single flip brings the valences closer to their targets.  No vertex moves, nv
 * and nf never change.  tests/mm_checkers/flip_edges.py is the executable form.  All f64 is unfused, in the order written;
 * len_sq is that of "mesh refinement", the cross components and dot are those of "surface distance".  One pass reads only
 * the state before it.
 *
 * Edge table.  Every corner pair of every face owns its undirected edge, as mm_mesh_refine counts: an owner count, and
 * first = the smallest corner id 3 f + j that names the edge.  deg[v] = the distinct edges lo != hi at v.  v is a border
 * vertex when it ends an edge, an (a, a) edge too, whose owner count is not 2.  ex[v] = deg[v] - (border ? 4 : 6).  The
 * deviation is the sum of ex[v] ex[v] over all vertices, an int64.
 *
 * Candidate.  An edge lo < hi is a candidate when all of these hold; they are tried in this order.
 *   (a) its owner count is 2 and the owners traverse it in opposite directions: F+ runs lo -> hi, F- runs hi -> lo.  Two
 *       owners of one direction make an inconsistent edge, which is counted and never flipped.
 *   (b) both owners have three distinct indices, and the opposite corners c (of F+) and d (of F-) differ.
 *   (c) mask[lo] == 0 and mask[hi] == 0, where a mask is given.
 *   (d) g = 2 (ex[lo] + ex[hi] - ex[c] - ex[d]) - 4 > 0: the exact drop of the deviation if this flip alone is made.
 *   (e) the edge c - d is not in the table.
 *   (f) n0 = (hi-lo) x (c-lo), n1 = (lo-hi) x (d-hi), m0 = (d-lo) x (c-lo), m1 = (c-hi) x (d-hi): the normals of F+, F-
 *       and of the two faces the flip would make.  dot(m0,n0), dot(m0,n1), dot(m1,n0), dot(m1,n1) are all > 0.
 *   (g) dn = dot(n0,n1) > 0 and dn dn >= (crease_cos crease_cos) (dot(n0,n0) dot(n1,n1)).
 *   (h) q(i,j,k; n) = dot(n,n) / (S S), S = (len_sq(i,j) + len_sq(j,k)) + len_sq(k,i), 0 where S == 0, a true division:
 *       q0 = q(lo,d,c; m0), q1 = q(hi,c,d; m1), t0 = k2 q(lo,hi,c; n0), t1 = k2 q(hi,lo,d; n1) with k2 = quality_keep
 *       quality_keep; q0 >= t0, q0 >= t1, q1 >= t0 and q1 >= t1 -- min(q0, q1) >= k2 min(q(n0), q(n1)), written so that a
 *       NaN fails.
 * A NaN fails whichever comparison it meets.  Of (e) .. (h) the first that fails is counted: blocked_existing, _normal,
 * _crease, _quality, summed over the passes.
 *
 * Selection.  A candidate has the priority min(g, 2^20) << 32 | (0xFFFFFFFF - first): unique per edge, never 0.  best[v] =
 * the largest priority among the candidates with v in {lo, hi, c, d}.  A candidate flips iff it is best at all four of
 * its vertices.  So flipped edges share no vertex, hence no face: every g is exact and the deviation falls by the sum of
 * the flipped g.  The largest priority of the mesh always flips, so a pass with a candidate flips something, and the
 * deviation, a non-negative integer, ends the passes.  Nothing depends on an order of visits.
 *
 * Rewrite, in place: F+ <- (lo, d, c), F- <- (hi, c, d).  Every other face keeps its bits and its place.
 *
 * Passes repeat until one has no candidate (converged) or max_passes have run.  passes_run counts the passes whose
 * candidates were sought: the last may have found none.
 *
 * Edges of the report, all of the input: n_edges between different vertices; open (one owner) and non-manifold (more than
 * two), (a, a) edges too; inconsistent as in (a); masked = the edges between different vertices with a nonzero mask byte
 * at either end.  The volumes are those of mm_refine_report.
 *
 * Device (mm_flip_kernels.hip; integer atomics only).  One upload: the vertices (24 nv), the faces as int32 (12 nf), the
 * mask where given (nv): bytes_uploaded.  The faces are rewritten where they lie; per pass the 128 bytes of counters are
 * read back.  One download: the faces and the counters, bytes_downloaded = 12 nf + 128.  Launches, with V = 1 + max(1,
 * ceil(ceil(log2 nf) / 8)) for a volume: a pass is 5 -- the edge table with owners and first corners, the valences with
 * the edge counts, the deviation, the candidates with their priorities, the flips.  Where no pass converged (max_passes
 * == 0 too) the valences of the result cost 3 more:
 *     n_launches = 2 V + 5 passes_run + (converged ? 0 : 3)
 * With nv == 0 or nf == 0 nothing is launched, the input is returned and both deviations are 36 nv.
 *
 * Limits as mm_mesh_refine: int32 indices, nv, nf < 2^31 and indices in [0, nv) (MM_ERR_INVALID), 6 nf < 2^31
 * (MM_ERR_TOO_LARGE).  crease_cos outside [0, 1], quality_keep outside [0, 1] or not finite, max_passes < 0:
 * MM_ERR_INVALID.  On an error no output is written. */

#define MM_FLIP_PASS_SLOTS 16

typedef struct mm_flip_report {
    int64_t n_vertices, n_faces;
    int64_t n_edges, n_open_edges, n_nonmanifold_edges, n_inconsistent_edges, n_masked_edges;
    int64_t passes_run, converged, n_flips;
    int64_t flips_per_pass[MM_FLIP_PASS_SLOTS];        /* passes beyond 16 add into the last slot                      */
    int64_t candidates_per_pass[MM_FLIP_PASS_SLOTS];
    int64_t blocked_existing, blocked_normal, blocked_crease, blocked_quality;
    int64_t deviation_before, deviation_after;
    int64_t n_launches, bytes_uploaded, bytes_downloaded;
    double  volume_before, volume_after;
} mm_flip_report;                                      /* 424 bytes */

/* The first half of a pass made public.  vertices_xyz is not read (nullable): the valences are the faces' alone.
 * out_degree[v] = deg[v], out_border[v] = 1 for a border vertex.  info[6] = {edges, open edges, non-manifold edges,
 * inconsistent edges, deviation, kernel launches (3)}.  With nv == 0 or nf == 0 nothing is launched. */
int     mm_mesh_valence(mm_engine* e, const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf,
                        int32_t* out_degree, uint8_t* out_border, int64_t* info);
/* The passes above.  mask (nullable): nv bytes.  crease_cos: the cosine of the largest angle between the normals of F+ and
 * F- across which an edge still flips.  max_passes == 0 returns the input with the edge counts, deviations and volumes
 * filled.  out_tris: nf triples (may be tris). */
int     mm_mesh_flip_edges(mm_engine* e, const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf,
                           const uint8_t* mask, double crease_cos, double quality_keep, int64_t max_passes,
                           int64_t* out_tris, mm_flip_report* report);

/* ---- mesh edge collapse (multimodars/ccta/fixing_functions.py:207-219: of MeshLab's isotropic remesh the collapse,
 *      collapseflag; MeshLab's midpoint collapse and its checksurfdist bound stay out; the repair is "mesh repair") ----------------------
 * Removes the short edges of a mesh (v, faces) by half-edge collapses r -> k: r and the two faces at the edge vanish, k
 * takes the place of r in the other faces at r, no surviving vertex moves.  The half-edge form is this project's choice,
 * not MeshLab's (which collapses onto the midpoint): it lets no measured vertex move; quality_keep is ours too.
 * tests/mm_checkers/collapse_edges.py is the executable form.  All f64 is unfused, in the order written; len_sq, the
 * cross components, dot and the quality q are those of "mesh edge flips".  A NaN fails whichever comparison it meets.
 * One pass reads only the state before it.
 *
 * Thresholds, each computed once: thr_min2 = (min_ratio L)(min_ratio L), thr_max2 = (max_ratio L)(max_ratio L), L =
 * target_len; min_ratio 4/5 and max_ratio 4/3 are those of Botsch and Kobbelt and of MeshLab, as the split's 4/3 is.
 *
 * Edge table: the owner counts, the two owner words with their direction bits, first, deg, border and "inconsistent" are
 * those of "mesh edge flips", over the faces still alive (a face killed by an earlier pass is not inserted; the corner ids
 * are those of the input).  nbr(x) = the other ends of the edges lo != hi at x.
 *
 * Removable vertex.  r is removable when mask[r] == 0, r is not a border vertex, no edge at r is inconsistent (two owners
 * of one direction; an (r, r) edge owned twice has both direction bits 0 and counts), and deg[r] >= 3.  Every face at a
 * removable r holds r once, and exactly one of them traverses r -> n for every n in nbr(r).
 *
 * Short edge: lo < hi with len_sq(lo, hi) < thr_min2.  A direction (r -> k), {r, k} = {lo, hi}, is admissible when
 *   (a) the edge has two owners of opposite directions, both with three distinct indices, and their opposite corners c
 *       (of F+, which runs lo -> hi) and d (of F-) differ;
 *   (b) r is removable -- k may be pinned or on a border: it neither moves nor vanishes;
 *   (c) link condition: nbr(r) and nbr(k) share exactly c and d;
 *   (d) valences after the collapse: deg[k] + deg[r] - 4 >= 3; deg[c] - 1 >= 3, >= 2 where c is a border vertex; the same
 *       for d (no tetrahedron, no vertex of valence 2);
 *   (e) for every n in nbr(r) \ {k, c, d}: len_sq(k, n) <= thr_max2 -- the split does not cut what the collapse makes;
 *   (f) for every face at r other than F+ and F-, rotated to (r, x, y): n_old = (x-r) x (y-r), n_new = (x-k) x (y-k), dn =
 *       dot(n_old, n_new) > 0 and dn dn >= (crease_cos crease_cos) (dot(n_old,n_old) dot(n_new,n_new)): no fold, and no
 *       crease such as the rim of a flat cap is flattened;
 *   (g) with k2 = quality_keep quality_keep: the smallest q(k,x,y; n_new) over those faces >= the smallest k2 q(r,x,y;
 *       n_old) over all faces at r, F+ and F- too; a NaN among the q of either side fails.
 * Every guard is a flag or an exact minimum / maximum over the ring: no order enters.  If both directions are admissible
 * the edge takes the one whose longest new edge (the largest len_sq(k, n) of (e), 0 without one) is shorter, r = hi on a
 * tie; else the admissible one.  It is then a candidate.
 *
 * A short edge without an admissible direction is counted once, summed over the passes: blocked_fixed where neither end is
 * removable; else blocked_link where (a) fails (the edge has no link of two vertices); else by the first class of (c) ..
 * (g) that fails for r = hi if hi is removable, else for r = lo: blocked_link, _valence, _long, _normal, _quality.  In
 * every pass the short edges are the candidates and the blocked ones.
 *
 * Selection.  A candidate has the priority ((0xFFFFFFFF - (bits(len_sq(lo, hi)) >> 32)) << 32) | (0xFFFFFFFF - first): the
 * shorter edge first, compared to 20 mantissa bits; unique per edge, never 0.  best[x] = the largest priority among the
 * candidates with x in {r} + nbr(r).  A candidate collapses iff it is best at every one of those vertices.  So the closed
 * stars of the removed vertices of a pass are pairwise disjoint: no two collapses create the same edge, and none changes
 * a neighbourhood, a degree or a face that another one read, so every guard is exact whatever else collapses.  The largest
 * priority of the mesh always collapses, so a pass with a candidate removes a vertex, and the vertex count ends the passes.
 *
 * Rewrite, in place: r <- k in every face at r; F+, F- and r die.  Every other face and every vertex keeps its bits.
 * After the last pass one stable compaction of vertices and faces: survivors keep their relative order.  origin[new] =
 * old; target[old] = the new index of the survivor the vertex ended in, chains across the passes followed.
 *
 * Passes repeat until one has no candidate (converged) or max_passes have run.  n_short_before / _after: the short edges
 * of the input and of the result.  The edge counts are those of the input, as mm_flip_report's.
 *
 * Device (mm_collapse_kernels.hip; integer atomics only).  One upload: the vertices (24 nv), the faces as int32 (12 nf),
 * the mask where given (nv): bytes_uploaded.  The vertices are never written, the faces are rewritten where they lie, dead
 * faces and vertices are marked; per pass the 128 bytes of counters are read back.  One download: the compacted vertices
 * and faces, origin, target and the counters, bytes_downloaded = 28 nv_out + 12 nf_out + 4 nv + 128.  Launches, with V(n)
 * = 1 + max(1, ceil(ceil(log2 n) / 8)) for a volume: a pass is 10 -- the edge table with owners and first corners, the
 * valences with the edge counts, the sorted adjacency (6), the candidates, the collapses.  Where no pass converged
 * (max_passes == 0 too) the table of the result costs 2 more.  The end is 9: two scans (3 each), the gather, the remap,
 * origin and target:
 *     n_launches = V(nf) + V(nf_out) + 10 passes_run + (converged ? 0 : 2) + 9
 * With nv == 0 or nf == 0 nothing is launched and the input is returned with origin = target = the identity.
 *
 * Limits as mm_mesh_flip_edges.  target_len not finite or not > 0, min_ratio outside (0, 1], max_ratio < 1 or not finite:
 * MM_ERR_INVALID.  On an error no output is written. */

#define MM_COLLAPSE_PASS_SLOTS 16

typedef struct mm_collapse_report {
    int64_t n_vertices, n_faces, n_vertices_out, n_faces_out;
    int64_t n_edges, n_open_edges, n_nonmanifold_edges, n_inconsistent_edges;
    int64_t n_short_before, n_short_after;
    int64_t passes_run, converged, n_collapses;
    int64_t collapses_per_pass[MM_COLLAPSE_PASS_SLOTS];    /* passes beyond 16 add into the last slot                  */
    int64_t candidates_per_pass[MM_COLLAPSE_PASS_SLOTS];
    int64_t blocked_fixed, blocked_link, blocked_valence, blocked_long, blocked_normal, blocked_quality;
    int64_t n_launches, bytes_uploaded, bytes_downloaded;
    double  volume_before, volume_after;
} mm_collapse_report;                                      /* 448 bytes */

/* The passes above.  mask (nullable): nv bytes, a nonzero byte pins the vertex.  out_vertices, out_origin: capacity nv;
 * out_tris: capacity nf triples; out_target: nv entries.  max_passes == 0 returns the input with the counts and volumes
 * filled. */
int     mm_mesh_collapse_edges(mm_engine* e, const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf,
                               const uint8_t* mask, double target_len, double min_ratio, double max_ratio,
                               double crease_cos, double quality_keep, int64_t max_passes, double* out_vertices,
                               int64_t* out_tris, int64_t* out_origin, int64_t* out_target, mm_collapse_report* report);

/* ---- mesh repair (multimodars/ccta/fixing_functions.py:114-239: the five MeshLab repair filters that stand in front of
 *      the hole filling and behind the isotropic remesh of fix_and_remesh_stitched_mesh) -----------------------------------
 * MeshLab and vcglib are not available to this project, so the rules are its own: they restate what the filters do as far
 * as that is known and make every choice deterministic.  tests/mm_checkers/repair_mesh.py is the executable form.
 *
 * Input: vertices (nv, 3) f64, all finite (magnitudes up to 2^250, so that q below stays finite); faces (nf, 3) with
 * indices in [0, nv).  The stages run in this order, each behind its flag.  A stage whose flag is off changes nothing but
 * still counts what it finds (n_welded_vertices, n_null_faces, n_duplicate_faces, n_nonmanifold_edges_before,
 * n_nonmanifold_vertices), which is what mm.mesh_manifold_report reads; n_faces_removed, n_new_vertices and
 * n_unreferenced_dropped count what was done.
 *
 * (a) Duplicate vertices (MM_REPAIR_DUPLICATE_VERTICES).  Two vertices are duplicates when all three coordinates compare
 *     equal with ==, so +0.0 equals -0.0; nothing is rounded, and unreferenced vertices take part (unlike
 *     mm_mesh_assemble).  Of a set of duplicates the smallest index survives with its own bits; rep[i] is that index.
 *     The faces are read through rep.
 * (b) Degenerate and null faces.  A face with a repeated index (through rep) is dropped whatever the flags say:
 *     n_degenerate_faces.  Of the others, with p0, p1, p2 the coordinates of its corners in face order, u = p1 - p0, w =
 *     p2 - p0, cx = uy wz - uz wy, cy = uz wx - ux wz, cz = ux wy - uy wx (two products and one subtraction each, unfused),
 *     q = (cx cx + cy cy) + cz cz: the squared double area.  A face with cx == 0, cy == 0 and cz == 0 is null
 *     (n_null_faces) and dropped with MM_REPAIR_NULL_FACES.
 * (c) Duplicate faces (MM_REPAIR_DUPLICATE_FACES).  Of the faces left with one vertex set, the smallest index stays with
 *     its own corner order, as in mm_mesh_assemble; the others are counted (n_duplicate_faces) and dropped.
 * (d) Non-manifold edges, by removing faces (MM_REPAIR_NONMANIFOLD_EDGES; MeshLab's method 0).  n_open_edges_before and
 *     n_nonmanifold_edges_before: the edges of the faces left with one owner and with more than two.  The faces that
 *     have an edge with more than two owners are visited in ascending order of the key (q, index) -- equal q: the
 *     smaller index first, which vcglib's std::sort leaves open --, and a face is deleted when its turn comes iff it
 *     still has such an edge.  The owners of one edge come in key order, so when the owner of rank r among c is
 *     visited at least c - r are left: the walk equals its closed form, which the device computes in one pass --
 *         a face is removed iff, on some edge with c > 2 owners, it is not one of the two owners with the largest keys.
 *     A face that one of its edges keeps and another removes goes, and may leave an open edge.  n_faces_removed;
 *     n_open_edges_after, n_nonmanifold_edges_after: the same counts of the faces left (the later stages keep them).
 * (e) Non-manifold vertices, by splitting (MM_REPAIR_NONMANIFOLD_VERTICES; MeshLab's displacement 0).  Corner 3 f + k
 *     is corner k of face f.  Two corners at one vertex are linked when their faces share an edge at that vertex that
 *     has exactly two owners, whatever the directions (the adjacency of mm_fix_winding); edges with other counts link
 *     nothing.  The corners at a vertex fall into components.  The component that holds the vertex's smallest corner
 *     keeps the vertex; every other one gets a new vertex with the parent's bits.  n_nonmanifold_vertices: the vertices
 *     with more than one component; n_new_vertices: the vertices made.  New vertices follow the vertices kept, in
 *     increasing order of their component's smallest corner (survivors keep their order, so input and output corner ids
 *     order alike).
 *     A weld that the split would only undo is not made.  Where a component that does not keep the vertex consists of
 *     exactly the corners of ONE input vertex w that stage (a) welded into the vertex -- every corner of the component is
 *     w's, and every corner w has in the faces left is in it --, the component gets no new vertex: w comes back, at its
 *     own place in the input order and with its own bits, is counted in neither n_welded_vertices nor n_new_vertices,
 *     and does not make its vertex count as non-manifold; origin and target name w itself.  This holds with the split
 *     switched off as well: stage (a) then creates no pinch.  So the output of a call is a mesh that needs nothing: a
 *     second call welds each vertex the split made to its parent, finds the same components and undoes every such weld.
 * (f) Unreferenced vertices (MM_REPAIR_DROP_UNREFERENCED; off in the Python default, MeshLab's five filters leave them):
 *     a survivor of (a) that no face left names is dropped, n_unreferenced_dropped.
 *
 * The order is not the reference's (edges, vertices, duplicate faces, duplicate vertices, null faces): with a
 * displacement of 0 its duplicate-vertex filter merges again what the split has just made.  Here the weld comes first and
 * the split last, so what the split separates stays separate, within a call and, by the undone welds of (e), across calls.
 *
 * Outputs: the vertices kept in input order, then the new ones; the faces left in input order with their own corner order,
 * renamed; origin[i] = the input vertex whose bits output vertex i carries; target[j] = the output vertex of input vertex
 * j through rep, -1 where (f) dropped it.  A mesh that needs nothing comes back bit for bit with origin = target = the
 * identity and every count 0.
 *
 * Device (mm_repair_kernels.hip; integer atomics only, no output depends on the order of arrival).  One upload (24 nv +
 * 12 nf = bytes_uploaded), one download (28 n_vertices + 12 n_faces + 4 nv + 152 = bytes_downloaded) and 4 bytes a
 * jumping round.  With nf > 0 a call launches MM_REPAIR_LAUNCHES kernels whatever the flags and the mesh -- (a) 2, (b)
 * and (c) 2, the edge table and its report 2, (d) 5, the table and report of the faces left 2, (e) the hook 1 and
 * 3, (f) 1, the three scans 9, the output 2 -- plus union_rounds pointer-jumping rounds of the corner union-find, each
 * one launch: n_launches = MM_REPAIR_LAUNCHES + union_rounds, and union_rounds <= 2 + ceil(log2(max(3 nf, 2))).
 * union_rounds is the one field that is not a function of the input alone (a round may or may not see a link another
 * lane moves).  With nf == 0 the scans over faces and corners and the rounds are not launched; with nv == 0 nothing is.
 *
 * Limits: nv, nf < 2^31 and 6 nf < 2^31 (MM_ERR_TOO_LARGE beyond); an index out of range, a non-finite coordinate or an
 * unknown flag bit: MM_ERR_INVALID, checked before anything is allocated.  tris: the nf faces; out_faces: capacity nf;
 * out_vertices and out_origin: capacity vert_cap; out_target: nv.  Where n_vertices > vert_cap nothing but the report is written and the
 * call returns MM_ERR_TOO_LARGE, the report complete: the protocol of mm_fill_holes. */

#define MM_REPAIR_DUPLICATE_VERTICES   1
#define MM_REPAIR_NULL_FACES           2
#define MM_REPAIR_DUPLICATE_FACES      4
#define MM_REPAIR_NONMANIFOLD_EDGES    8
#define MM_REPAIR_NONMANIFOLD_VERTICES 16
#define MM_REPAIR_DROP_UNREFERENCED    32
#define MM_REPAIR_ALL_FLAGS            63
#define MM_REPAIR_LAUNCHES             28

typedef struct mm_repair_report {
    int64_t n_vertices, n_faces;                           /* of the result                                            */
    int64_t n_welded_vertices, n_degenerate_faces, n_null_faces, n_duplicate_faces;
    int64_t n_nonmanifold_edges_before, n_nonmanifold_edges_after, n_faces_removed;
    int64_t n_nonmanifold_vertices, n_new_vertices, n_unreferenced_dropped;
    int64_t n_open_edges_before, n_open_edges_after;
    int64_t union_rounds, n_launches, bytes_uploaded, bytes_downloaded;
} mm_repair_report;                                        /* 144 bytes */

int     mm_mesh_repair(mm_engine* e, const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf, int flags,
                       int64_t vert_cap, double* out_vertices, int64_t* out_faces, int64_t* out_origin,
                       int64_t* out_target, mm_repair_report* report);

/* ---- mesh intersections (multimodars/ccta/fixing_functions.py:182-185, 234: meshing_close_holes(selfintersection=False),
 *      the question the reference leaves to MeshLab and switches off) ---------------------------------------------------
 * Which pairs of faces of one mesh (the self form), or of two, pass through each other.  tests/mm_checkers/
 * mesh_intersections.py is the executable form of the rule; csrc/mm_isect_device.h is its C++ text.
 *
 * Every pair of faces is DISJOINT (0), INTERSECTING (1) or UNDECIDED (2).  A state other than UNDECIDED is a proof in
 * exact arithmetic on the f64 inputs: DISJOINT by a separating witness, INTERSECTING by a strict crossing.  UNDECIDED is
 * what the filtered predicates cannot prove: touching or coplanar within rounding.  The state is a pure function of the
 * two faces' coordinates and vertex identities, computed in unfused f64 in the order written below, so chunking,
 * scheduling and culling cannot change a bit.  In the self form face 1 of a pair is the one with the lower index; in the
 * two-mesh form it is the face of mesh a.
 *
 * 1. Vertex identity (self form).  The canonical id of a vertex is the lowest index with equal coordinates, +0.0 == -0.0
 *    as in "mesh repair": an unwelded seam reads as adjacent.  The two-mesh form has no identities.
 * 2. A degenerate face -- two equal canonical ids, or every component of ab x ac exactly 0.0 as in "surface distance" -- is
 *    counted, tested against nothing, and has state 0.
 * 3. Box step.  Closed coordinate boxes of the two faces disjoint on an axis: DISJOINT.  Corners lie in their boxes
 *    exactly, so there is no slack, and a cull by the boxes of groups of faces loses nothing.
 * 4. Predicates, sign +1, -1 or 0 = not certain; eps = 2^-53.
 *    orient3d(a,b,c,d): adx = ax-dx ... cdz = cz-dz; det = (adz*(bdx*cdy - cdx*bdy) + bdz*(cdx*ady - adx*cdy)) +
 *    cdz*(adx*bdy - bdx*ady); permanent = ((|bdx*cdy| + |cdx*bdy|)*|adz| + (|cdx*ady| + |adx*cdy|)*|bdz|) +
 *    (|adx*bdy| + |bdx*ady|)*|cdz|; certain iff |det| > (7 + 56 eps) eps * permanent (stage A of Shewchuk's orient3d).
 *    orient2d(a,b,c) on the two coordinates left when the axis of the largest |component| of face 1's normal
 *    (q1-p1) x (r1-p1) is dropped (the first of equal ones; x drops to (y, z), y to (x, z), z to (x, y)):
 *    left = (au-cu)*(bv-cv), right = (av-cv)*(bu-cu), det = left - right, detsum = |left| + |right|; certain iff
 *    |det| > (3 + 16 eps) eps * detsum.  A permanent or detsum that is not finite or is below 2^-900 is not certain.
 * 5. No shared vertex.  a_k = orient3d(p1,q1,r1, corner k of face 2): all three certain and equal: DISJOINT; then b_k =
 *    orient3d(p2,q2,r2, corner k of face 1) likewise.  All six not certain: in the projection of 4., DISJOINT if an edge
 *    of one triangle (inner side certain) has the other's three corners certainly on its outer side -- face 1's edges pq,
 *    qr, rp first, then face 2's -- else UNDECIDED.  Any of the six not certain: UNDECIDED.  Otherwise rotate each face so
 *    that the corner whose sign differs from the other two comes first (Guigue-Devillers); if that corner of face 1 is
 *    negative swap q2, r2, if that of face 2 is negative swap q1, r1; e1 = orient3d(p1,q1,p2,q2): positive: DISJOINT;
 *    e2 = orient3d(p1,r1,r2,p2): positive: DISJOINT; both negative: INTERSECTING; else UNDECIDED.
 * 6. One shared vertex.  Rotate each face so that it comes first.  q1, r1 certainly on one side of face 2's plane:
 *    DISJOINT; q2, r2 against face 1's likewise.  The segment q1 r1 against face 2: crossing iff its ends are certainly
 *    on opposite sides and orient3d(q1,r1,p2,q2), (q1,r1,q2,r2), (q1,r1,r2,p2) are certain and equal; missing iff two of
 *    those three are certainly opposite.  Crossing: INTERSECTING; else q2 r2 against face 1 likewise; both missing:
 *    DISJOINT.  Else, with all four plane signs not certain (a flat pair, as the children of a refined face), in the
 *    projection of 4. taken on the rotated face 1: DISJOINT if one of the edges at the shared vertex -- p1 q1, r1 p1,
 *    p2 q2, r2 p2 in that order -- has its inner side certain and the other face's two far corners certainly on its
 *    outer side; else UNDECIDED.
 * 7. Two shared vertices.  The unshared corner of face 2 certainly off face 1's plane, or that of face 1 off face 2's:
 *    DISJOINT.  Else, with (c1, a, b) face 1 rotated so that its unshared corner comes first, orient2d(a,b,c1) and
 *    orient2d(a,b,c2) certain and opposite: DISJOINT (a flat pair); else UNDECIDED (a fold-over).
 * 8. Three shared vertices: INTERSECTING, counted in n_coincident_pairs. */

typedef struct mm_intersect_report {
    int64_t n_intersecting_pairs, n_undecided_pairs;
    int64_t n_degenerate_faces;   /* of both meshes */
    int64_t n_coincident_pairs;   /* among the intersecting ones */
    int64_t items;                /* chunk pairs whose boxes overlap: the workgroups that ran */
    int64_t items_total;          /* chunk pairs before the cull */
    int64_t pair_box_tests;       /* face pairs inside the items */
    int64_t narrow_tests;         /* face pairs that passed the box step: the same whatever the cull */
    int64_t n_launches, bytes_uploaded, bytes_downloaded;
    int64_t pairs_complete;       /* 0: more pairs than max_pairs, no list */
} mm_intersect_report;

/* vb == NULL selects the self form (nvb, fb, nfb are not read, out_state_b not written).  out_state_a / out_state_b: one
 * byte per face, bit 0 = in an intersecting pair, bit 1 = in an undecided one.  out_pairs (2 per pair, original face
 * indices: i < j in the self form, (face of a, face of b) otherwise; rows ascending) and out_pair_state (1 or 2) hold at
 * most max_pairs pairs and may be NULL (then max_pairs counts as 0); with more pairs than that nothing is written to
 * them and pairs_complete is 0, the counts and flags are complete all the same.  Empty meshes are valid.
 * MM_ERR_INVALID: a non-finite coordinate, a face index out of range, a size of 2^31 or more; MM_ERR_TOO_LARGE: more
 * than 2^31 - 1 items.  On an error the outputs are not written. */
int     mm_mesh_intersections(mm_engine* e, const double* va, int64_t nva, const int64_t* fa, int64_t nfa, const double* vb,
                              int64_t nvb, const int64_t* fb, int64_t nfb, int64_t max_pairs, uint8_t* out_state_a,
                              uint8_t* out_state_b, int64_t* out_pairs, int8_t* out_pair_state, mm_intersect_report* report);
/* TEST HOOK (nothing in the product calls it; no engine, no device): the host side of mm_mesh_intersections.
 * order_a[j] / order_b[j] = the face staged at position j (slabs by corner sum across the longest axis of all corners).
 * chunk_boxes (nullable): lo xyz, hi xyz of every chunk of a, then of b.  items (2 int32 each: chunk I of a, chunk J of b
 * or, in the self form, of a with I <= J) receives at most cap items.  info[5] = {items, chunk pairs before the cull,
 * faces per chunk, chunks of a, chunks of b}.  Errors as mm_mesh_intersections. */
int     mm_isect_plan(const double* va, int64_t nva, const int64_t* fa, int64_t nfa, const double* vb, int64_t nvb,
                      const int64_t* fb, int64_t nfb, int32_t* order_a, int32_t* order_b, int64_t* info, double* chunk_boxes,
                      int32_t* items, int64_t cap);

/* ---- mesh cross-sections (no counterpart in the reference, whose roadmap lists "assess lumen area, minor-, major axis,
 *      mla ... from the CCTA mesh" as open) ---------------------------------------------------------------------------
 * The exact intersection of a triangle mesh with P planes, as contours with their measures.  tests/mm_checkers/
 * mesh_sections.py is the executable form of the rule; csrc/mm_section_device.h is the C++ text of rules 1-4 and 8,
 * csrc/mm_section.cpp that of rules 5-7.
 *
 * Inputs: v f64[nv,3], f int64[nf,3]; per plane an origin o and a normal n, which need not be unit.  Everything is
 * unfused f64 in the order written, so chunking, scheduling, the cull and the order of the faces cannot change a bit of
 * a point or a measure.
 *
 * 1. Height and side.  h(x) = (nx*(x.x-o.x) + ny*(x.y-o.y)) + nz*(x.z-o.z); side(x) = 0 if h < 0, else 1: a vertex
 *    exactly on the plane is above it.  This is the whole degeneracy policy: the side is a function of the vertex alone,
 *    so every face that shares it agrees, a plane through a vertex, an edge or a whole face needs no special case, and
 *    every crossed face has exactly two crossed edges.
 * 2. Faces.  A face with a repeated index is skipped and counted (n_skipped_faces).  Every other face is crossed by a
 *    plane iff its three sides are not equal; faces without area are included.  Vertex identity is the index, not the
 *    coordinates: an unwelded seam cuts into open polylines (mm_mesh_repair welds it).
 * 3. Crossing point of a crossed edge.  The edge is keyed (lo, hi) by vertex index, lo < hi, and its point is always
 *    computed from lo to hi: t = h_lo / (h_lo - h_hi); p = v_lo + t*(v_hi - v_lo) per component.  The two faces of an
 *    edge compute the same bits.  One height is < 0 and the other >= 0, so the denominator is never 0 and 0 <= t <= 1.
 * 4. Segment.  One per (plane, crossed face): the plane, the face, its two edge keys, the smaller key first (by lo, then
 *    by hi), and the two points in that order.
 * 5. Chaining, per plane, of its segments in ascending face order.  Segments that share an edge key are joined; a
 *    component is a connected set of them.
 *    - Some edge key has more than two segments: BRANCHED (kind 2).  Its distinct points are listed in ascending edge-key
 *      order, with point_face = -1; area and centroid are NaN; length = the sum of its segments' lengths |p1 - p0| in
 *      ascending face order.
 *    - Two keys of one segment each: OPEN (kind 1), listed from the end with the smaller key.
 *    - Every other component: a CLOSED loop (kind 0), listed from its smallest edge key, leaving it towards the smaller
 *      of the two neighbouring keys (by the segment of the smaller face where both lead to the same key).  s (rule 6) is
 *      computed in this order; if s < 0 the loop is listed the other way round (p0, p(m-1), ..., p1) and rule 6 is
 *      computed anew in that order, whose s is the one reported; at s >= 0 the first order stays.
 *    point_face of a point is the face of the segment that leaves it, -1 at the far end of an open polyline.  The
 *    components of a plane are ordered by their smallest edge key.
 * 6. Measures, with p(m) = p(0) for a loop, from i = 0, every sum started at 0.0:
 *    d_i = p_i - p_0, the loop's own first listed point (the same point in both directions), so that no measure depends
 *    on where o lies in its plane; c_i = d_i x d_(i+1) = (dy*ez - dz*ey, dz*ex - dx*ez, dx*ey - dy*ex) with e = d_(i+1);
 *    A += c_i; w_i = (c.x*nx + c.y*ny) + c.z*nz; W += w_i; G += w_i * (d_i + d_(i+1)) per component;
 *    q_i = (|dy*ez| + |dz*ey|, |dz*ex| + |dx*ez|, |dx*ey| + |dy*ex|); B += (q.x*|nx| + q.y*|ny|) + q.z*|nz|.
 *    s = (A.x*nx + A.y*ny) + A.z*nz; area = (0.5 * s) / sqrt((nx*nx + ny*ny) + nz*nz).
 *    len_i = sqrt((ex*ex + ey*ey) + ez*ez) with e = p_(i+1) - p_i; length L += len_i; M += len_i * (0.5 * (p_i + p_(i+1))).
 *    A loop is flat iff not |W| > ((m + 6) * 2^-52) * B: W differs from its exact value by at most (m + 6) * 2^-53 * B
 *    (DESIGN 4.28), so W of a loop that is not flat has its sign and is within a factor 2 of the truth.
 *    centroid = p_0 + G / (3.0 * W) per component, the area centroid of the fan about p_0; of a flat loop it is M / L,
 *    the length-weighted mean, and p_0 where L == 0.  An open polyline (its m - 1 segments) has length L and centroid
 *    M / L (p_0 where L == 0); its area is NaN.
 * 7. Selection.  Drop the axis of the largest |n| component, the first among equals (x leaves (u, v) = (y, z), y leaves
 *    (x, z), z leaves (x, y)), as in rule 4 of "mesh intersections".  o is inside a closed loop iff the number of its
 *    segments (a, b) with (a.v > o.v) != (b.v > o.v) and o.u < a.u + ((o.v - a.v) * (b.u - a.u)) / (b.v - a.v) is odd
 *    (half-open in v).  selected[p] = among the closed loops of plane p that hold o the one with the smallest area (a
 *    lumen inside a wall), the first of equal ones; -1 if there is none.
 * 8. The cull loses nothing, with no slack.  h is monotone in each coordinate of x under rounding, so over a box it takes
 *    its extremes at the two corners the signs of n pick: h_min at (n.k < 0 ? hi.k : lo.k), h_max at the opposite corner.
 *    A chunk of 256 faces in slab order takes part for a plane iff h_min < 0 and not h_max < 0.  Heights
 *    that overflow are outside the rule. */

#define MM_SECTION_CLOSED   0
#define MM_SECTION_OPEN     1
#define MM_SECTION_BRANCHED 2
#define MM_SECTION_SEGMENT_BYTES 72

typedef struct mm_section_report {
    int64_t n_planes, n_faces;
    int64_t n_skipped_faces;      /* faces with a repeated index */
    int64_t n_segments;           /* (plane, crossed face) pairs: complete also where the call returns MM_ERR_TOO_LARGE */
    int64_t n_contours, n_closed, n_open, n_branched;
    int64_t items;                /* (plane, chunk) pairs that pass rule 8 */
    int64_t items_total;          /* planes x chunks */
    int64_t face_tests;           /* (plane, face) pairs inside the items */
    int64_t n_launches, bytes_uploaded, bytes_downloaded;
} mm_section_report;              /* 112 bytes */

/* Contours of every plane, plane after plane (plane_off: n_planes + 1 entries into the contours; selected: n_planes
 * contour indices or -1).  contour_off (one more entry than contours) indexes points (3 doubles), point_edge (2 int64:
 * lo, hi) and point_face.  The contour arrays hold max_segments entries (contour_off one more), the point arrays
 * 2 max_segments: no result is larger.  With more segments than max_segments the call returns MM_ERR_TOO_LARGE with
 * report->n_segments set and no other output written: call once more with that capacity.  An empty mesh and zero planes
 * are valid.  MM_ERR_INVALID: a non-finite coordinate or origin, a normal that is zero or not finite, a face index out
 * of range, a size of 2^31 or more. */
int     mm_mesh_sections(mm_engine* e, const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf,
                         const double* origins, const double* normals, int64_t n_planes, int64_t max_segments,
                         int64_t* contour_off, double* points, int64_t* point_edge, int64_t* point_face,
                         int64_t* contour_plane, int8_t* contour_kind, double* contour_area, double* contour_length,
                         double* contour_centroid, int64_t* plane_off, int64_t* selected, mm_section_report* report);
/* TEST HOOK (nothing in the product calls it; no engine, no device): the host plan of mm_mesh_sections.  order[j] = the
 * face staged at position j (slabs by corner sum across the longest axis of all corners); chunk_boxes (nullable): lo xyz,
 * hi xyz of every chunk; plane_list: per chunk, ascending, the planes that pass rule 8, chunk after chunk, at most
 * list_cap entries; items (4 int32 each: chunk, first entry of the run in plane_list, planes of the run, 0), at most
 * item_cap of them.  info[8] = {(plane, chunk) pairs, planes x chunks, faces per chunk, chunks, items, planes per run,
 * face tests, skipped faces}. */
int     mm_section_plan(const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf, const double* origins,
                        const double* normals, int64_t n_planes, int32_t* order, int64_t* info, double* chunk_boxes,
                        int32_t* plane_list, int64_t list_cap, int32_t* items, int64_t item_cap);
/* TEST HOOK (no engine, no device): the items of that plan cut on the host by the arithmetic the kernel runs
 * (csrc/mm_section_device.h).  segments: at most cap records of MM_SECTION_SEGMENT_BYTES (uint64 plane << 32 | face;
 * 4 int32: the two edge keys; 6 doubles: the two points), sorted by (plane, face); *n_segments = their full number. */
int     mm_section_cut_host(const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf, const double* origins,
                            const double* normals, int64_t n_planes, int64_t cap, void* segments, int64_t* n_segments);
/* TEST HOOK (no engine, no device): rules 5 to 7 on segment records sorted by (plane, face) -- the code
 * mm_mesh_sections runs on what the device returns.  The arrays as there, with n_segments in the place of max_segments.
 * counts[5] = {contours, points, closed, open, branched}. */
int     mm_section_chain(const void* segments, int64_t n_segments, const double* origins, const double* normals,
                         int64_t n_planes, int64_t* contour_off, double* points, int64_t* point_edge, int64_t* point_face,
                         int64_t* contour_plane, int8_t* contour_kind, double* contour_area, double* contour_length,
                         double* contour_centroid, int64_t* plane_off, int64_t* selected, int64_t* counts);

/* ---- mesh clipping (no counterpart in the reference, whose paper names "patient-specific CFD and FSI simulations" as
 *      the first use of its surface: a solver wants flat inlets and outlets) ------------------------------------------
 * A mesh cut open along plane sections: the crossed faces are split along a section's loop, one side of the loop is
 * thrown away by connectivity, the rim is left open, capped, or extended by a straight piece, and every face says which
 * patch it belongs to.  tests/mm_checkers/mesh_clip.py is the executable form of the rule; csrc/mm_clip_device.h is the
 * C++ text of C4's per-face step, csrc/mm_clip.cpp that of C1, C5 and C6, csrc/mm_clip_kernels.hip that of C2, C4, C7.
 *
 * Inputs: v f64[nv,3], f int64[nf,3] and K cuts, each an origin o, a normal n (need not be unit), keep in {BELOW (the
 * side h < 0 stays), ABOVE (h >= 0 stays)} and scope in {LOOP, PLANE}; cap (0/1), ext_length >= 0 and ext_layers >= 0
 * (both zero: no extension).  All arithmetic is unfused f64 in the order written.  Heights, sides, crossing points,
 * chaining, measures and selection are rules 1-7 of "mesh cross-sections", unchanged.
 *
 * C1. Cut set.  The sections of the K planes are taken.  LOOP: the faces of the segments of selected[k], the smallest
 *     closed loop around o; no such loop, or one of fewer than 3 points: status NO_LOOP.  PLANE: every crossed face of
 *     plane k (rules 1 and 2); its loop points are those of every contour of the plane.  A face in the cut sets of two
 *     cuts gives both status OVERLAP.  The measures reported for a cut are those of its first closed loop in contour order
 *     (LOOP: the selected one), NaN without one.  Where C1 leaves a status other than OK, C2 is not run.
 * C2. Connectivity.  A union-find over the vertex indices: a face in no cut set unites its three vertices, a face in a
 *     cut set only the two on the same side of its plane.  For every cut face of a LOOP cut the root of its apex (C4) is
 *     compared with the root of the next corner, one on the kept and one on the drop side: equal, the cut is
 *     NOT_SEPARATING; otherwise the drop-side root is marked.  A vertex is dropped iff its root is marked or it lies on
 *     the drop side of a PLANE cut.  Only root equality and the marks are used, never which member is the root.
 *     Where C2 leaves every status OK: a cut face whose kept-side old vertices (the apex where the apex is kept,
 *     otherwise b and c) include a dropped vertex is orphaned, and its cut gets status KEPT_SIDE_DROPPED: another cut
 *     throws away the side this one keeps, and its rim would be emitted joined to nothing.  A cut that is
 *     NOT_SEPARATING stays so: the orphan check reads the marks only after a verdict that left every status OK.
 * C3. All or nothing.  If any status is not OK nothing is cut: the outputs are the input mesh with identity maps,
 *     n_applied = 0, no rims, and the statuses and measures are reported.
 * C4. Pieces.  A face in no cut set is kept iff none of its vertices is dropped.  A cut face (c0, c1, c2) is rotated,
 *     winding preserved, to (a, b, c) with a, the apex, the vertex alone on its side (a = c2 if side(c0) == side(c1), c1
 *     if side(c0) == side(c2), else c0).  m_ab and m_ca are the loop points on the edges (a, b) and (c, a): the section's
 *     points, same bits.  Pieces, in this order: the apex piece (a, m_ab, m_ca); then the quad m_ab, b, c, m_ca cut by
 *     its shorter diagonal, with d2(p, q) = ((dx*dx + dy*dy) + dz*dz): if d2(m_ab, c) < d2(b, m_ca): (m_ab, b, c),
 *     (m_ab, c, m_ca); otherwise, ties included: (m_ab, b, m_ca), (b, c, m_ca).  A piece is kept iff none of its old
 *     vertices is dropped.  A piece with two corners of equal coordinates is emitted and counted (n_null_pieces): a vertex
 *     on a plane counts as above it, so such pieces are legitimate; mm_mesh_repair removes them.
 * C5. Vertices, in this order: the kept old vertices, bits and relative order unchanged; then per cut, in cut order, its
 *     loop points in the section's listing order (every contour of its cut set, in contour order), then rings
 *     1..ext_layers, each the points of the cut's closed loops in that order, then, with cap, one centre per closed
 *     loop.  vertex_origin is the old index, or -1 - k for a vertex made for cut k.
 * C6. Extension and cap, for every closed loop of every applied cut; open and branched contours of a PLANE cut stay open
 *     and are counted (n_open_loops).  u = n / sqrt((nx*nx + ny*ny) + nz*nz) per component; sgn = +1 where the dropped
 *     side is above (keep BELOW), else -1; step = ext_length / ext_layers.  The point of ring j is
 *     p + (sgn * (j * step)) * u per component.  The centre is the loop's rule-6 centroid shifted the same way by
 *     ext_layers * step; without an extension it is the centroid's bits.  For rim edge i (p_i, p_(i+1); the segment of
 *     point_face[i]) the kept side of that face runs along the edge x -> y: m_ab -> m_ca where the apex is kept, m_ca ->
 *     m_ab otherwise.  Faces: per layer j = 0..ext_layers-1 (ring 0 = the rim) (y_j, x_j, x_(j+1)) and
 *     (y_j, x_(j+1), y_(j+1)); the cap face (y_L, x_L, centre) with L = ext_layers.  The orientation follows the adjacent
 *     piece edge by edge and assumes no oriented mesh.
 * C7. Faces, in this order: the kept faces and pieces in parent order (a face's pieces in C4's order); per cut its
 *     extension faces, layer-major, in rim order (loop after loop, edge i after edge i - 1); per cut its cap faces in
 *     rim order.  face_origin is the parent face, or -1 - k; face_kind 0 untouched, 1 piece, 2 extension, 3 cap.
 * C8. Report: mm_clip_report, and per cut status, loop points, closed loops, cut faces (cut_status, 4 int64 a cut) and
 *     area, perimeter, centroid (cut_measures, 5 doubles a cut).
 *
 * Launches of the clip's own device pass (the section pass before it is mm_mesh_sections'): none without a cut, without
 * a vertex or with a status C1 set; otherwise 5 + R (initialise, scatter, sides, unions, R pointer-jumping rounds
 * including the one that changes nothing, verdict); where no cut is NOT_SEPARATING 1 more (the orphan check); and where
 * the cuts are applied 11 more (keep flags, 3 of their scan, piece counts, 3 of their scan -- none on a mesh without
 * faces: 8 --, vertices, faces, rim faces).  bytes_downloaded: 4 R + 4 K with a cut NOT_SEPARATING, otherwise 4 R + 8 K
 * (the K status words are read once after the verdict and once after the orphan check), and where the cuts are applied
 * 16 + 64 + 28 n_vertices + 17 n_faces more. */

#define MM_CLIP_KEEP_BELOW 0
#define MM_CLIP_KEEP_ABOVE 1
#define MM_CLIP_SCOPE_LOOP  0
#define MM_CLIP_SCOPE_PLANE 1
#define MM_CLIP_OK             0
#define MM_CLIP_NO_LOOP        1
#define MM_CLIP_OVERLAP        2
#define MM_CLIP_NOT_SEPARATING 3
#define MM_CLIP_KEPT_SIDE_DROPPED 4
#define MM_CLIP_KIND_UNTOUCHED 0
#define MM_CLIP_KIND_PIECE     1
#define MM_CLIP_KIND_EXTENSION 2
#define MM_CLIP_KIND_CAP       3

typedef struct mm_clip_report {
    int64_t n_cuts, n_applied;    /* n_applied: n_cuts where every status is OK, else 0 */
    int64_t n_vertices, n_faces;  /* of the result: the capacities needed where the call returns MM_ERR_TOO_LARGE */
    int64_t n_new_vertices;       /* loop points, ring points and centres */
    int64_t n_dropped_vertices;
    int64_t n_dropped_faces;      /* input faces of which nothing is left */
    int64_t n_cut_faces;
    int64_t n_pieces, n_null_pieces;
    int64_t n_ext_faces, n_cap_faces;
    int64_t n_closed_loops;       /* the rims */
    int64_t n_open_loops;         /* open and branched contours of PLANE cuts: left as they are */
    int64_t jump_rounds;          /* R */
    int64_t n_launches, bytes_uploaded, bytes_downloaded;   /* of the clip's own device pass */
} mm_clip_report;                 /* 144 bytes */

/* keep and scope: n_cuts int32 each.  out_vertices (3 doubles) and vertex_origin hold vert_cap entries, out_tris (3
 * int64), face_origin and face_kind face_cap; rim_off holds vert_cap + 1 entries and rim_index vert_cap: rim r, the
 * outermost ring of closed loop r (cut after cut, loop after loop), is rim_index[rim_off[r] .. rim_off[r + 1]), vertex
 * indices of the result in loop order; n_closed_loops of them.  cut_status: 4 int64 a cut, cut_measures: 5 doubles a
 * cut (C8).  Capacities as mm_mesh_refine: too small, report->n_vertices and n_faces hold the sizes needed, nothing else
 * is written and the call returns MM_ERR_TOO_LARGE.  An empty mesh and zero cuts are valid.  MM_ERR_INVALID, before the
 * engine's buffers are touched: a non-finite coordinate or origin, a zero or non-finite normal, a face index out of
 * range, a keep, scope or cap outside its values, a negative or non-finite ext_length, ext_layers < 0 (or above 2^20),
 * exactly one of ext_length and ext_layers zero, a size of 2^31 or more.  int32 indices on the device: a result of 2^31
 * or more vertices or faces is MM_ERR_TOO_LARGE. */
int     mm_mesh_clip(mm_engine* e, const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf,
                     const double* origins, const double* normals, const int32_t* keep, const int32_t* scope, int64_t n_cuts,
                     int32_t cap, double ext_length, int64_t ext_layers, int64_t vert_cap, int64_t face_cap,
                     double* out_vertices, int64_t* out_tris, int64_t* vertex_origin, int64_t* face_origin, int8_t* face_kind,
                     int64_t* cut_status, double* cut_measures, int64_t* rim_off, int64_t* rim_index, mm_clip_report* report);
/* TEST HOOK (nothing in the product calls it; no engine, no device): the same rule in host C++ -- the sections by
 * mm_section_cut_host and mm_section_chain, a sequential union-find, csrc/mm_clip_device.h for the pieces.  jump_rounds,
 * n_launches and the byte counts stay 0. */
int     mm_mesh_clip_host(const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf, const double* origins,
                          const double* normals, const int32_t* keep, const int32_t* scope, int64_t n_cuts, int32_t cap,
                          double ext_length, int64_t ext_layers, int64_t vert_cap, int64_t face_cap, double* out_vertices,
                          int64_t* out_tris, int64_t* vertex_origin, int64_t* face_origin, int8_t* face_kind,
                          int64_t* cut_status, double* cut_measures, int64_t* rim_off, int64_t* rim_index,
                          mm_clip_report* report);

/* ---- winding number (no counterpart in the reference, whose roadmap lists "write a more stable function to find
 *      intramural points on aorta" and "intramural length etc. from the CCTA mesh" as open) -----------------------------
 * The generalized winding number (Jacobson et al. 2013) of a triangle mesh at query points,
 * w(p) = (1 / 4 pi) sum_f Omega_f(p): 1 inside and 0 outside a closed mesh of positive volume (mm_fix_winding leaves it
 * so), a smooth fraction near the openings of an open one, where w > 1/2 stays a sound "inside".
 * tests/mm_checkers/winding_number.py is the executable form of the rule; csrc/mm_winding_device.h is its C++ text.
 * Everything is unfused f64 in the order written; dot(u, v) = (ux*vx + uy*vy) + uz*vz.  No atan2 runs on the device.
 *
 * 1. Staging.  Faces are taken in the caller's order.  Degenerate faces ("surface distance": a repeated index, or every
 *    component of ab x ac exactly 0.0) are removed first: a mesh with them gives the bits of the mesh without them.  nf'
 *    is the number of staged faces.  A coordinate of magnitude above 2^300 is an argument error, so L (2) stays finite.
 * 2. Per query p and staged face (A, B, C): a = A-p, b = B-p, c = C-p; la = sqrt(dot(a,a)), lb, lc likewise;
 *    L = (la*lb)*lc; u = b x c = (by*cz - bz*cy, bz*cx - bx*cz, bx*cy - by*cx); num = (ax*ux + ay*uy) + az*uz;
 *    den = ((la*lb)*lc + dot(a,b)*lc) + (dot(b,c)*la + dot(c,a)*lb).  Van Oosterom-Strackee:
 *    Omega_f / 2 = arg(den + i num), in (-pi, pi].
 * 3. A running angle is a pair (n, P): n an integer number of quarter turns, P = (pr, pi) a complex number in the cone
 *    pr >= |pi|; it stands for n*pi/2 + arg P.  cone(re, im) rotates a complex number into the cone by an exact multiple m
 *    of 90 degrees; the first case that holds:
 *      im > re && im >= -re && im > 0:   m = 1,  (im, -re)
 *      im < -re && im <= re && im < 0:   m = -1, (-im, re)
 *      re < 0:                           m = 2 where im >= 0, else -2; (-re, -im)
 *      otherwise:                        m = 0,  (re, im).
 * 4. To add m quarter turns and a z = (zr, zi) of the cone to (n, P): qr = pr*zr - pi*zi, qi = pr*zi + pi*zr;
 *    (m2, qr, qi) = cone(qr, qi) -- both factors lie in the cone and rounding is monotone, so qr >= 0 before the call and
 *    |m2| <= 1; n += m + m2; P = (qr, qi) scaled by the power of two that puts qr in [1/2, 1) (frexp, ldexp: exact).
 *    A face is folded with (m, z) = cone(den, num).  Two partial angles fold the same way: the second one's n is m, its P
 *    is z.
 * 5. Flags of a face, folded per query: touch (OR): den <= 0 && |num| <= 2^-47 * L -- the sign of num is not proven (the
 *    bound is Shewchuk's orient3d A-bound (7 + 56 eps) eps times a permanent of at most 6 L), so the face may lie on
 *    either side of its +-2 pi jump.  rho (min): max(|den|, |num|) / L, a true division: how far den + i num is from 0
 *    relative to its scale; small exactly when p is near the face's edges or corners.
 * 6. The zero face: max(|den|, |num|) < 2^-600, or the least of dot(a,a), dot(b,b), dot(c,c) < 2^-960 (a query on a
 *    vertex, and everything that could underflow).  It is not folded and sets rho = 0.
 * 7. Grouping, which fixes the bits.  A chunk is 256 consecutive staged faces; a group is G = ceil(chunks / 16)
 *    consecutive chunks, so there are ceil(chunks / G) <= 16 groups (mm_winding_plan reports the numbers).  A group's
 *    partial is the sequential fold of its faces from n = 0, P = (1, 0), rho = +inf, touch = 0; a query's total is the
 *    fold of its group partials in ascending order, the first one taken as it is.  G depends on nf' alone, so a query's
 *    bits do not depend on which other queries share the call.
 * 8. Result (host): w = (n * (pi/2) + atan2(pi, pr)) / (2 pi) with the C library's atan2.
 *    err = nf' * (MM_WINDING_ERR_C1 + MM_WINDING_ERR_C2 / rho) * 2^-53, a proven bound on |w - w_exact| for the f64 inputs
 *    (DESIGN 4.29); +inf where touch is set or rho < MM_WINDING_RHO_MIN (rho == 0 included).  Without a staged face
 *    w = 0, err = 0. */

#define MM_WINDING_ERR_C1  4.0
#define MM_WINDING_ERR_C2  9.0
#define MM_WINDING_RHO_MIN 9.094947017729282379150390625e-13   /* 2^-40 */

typedef struct mm_winding_report {
    int64_t n_staged_faces;       /* nf' */
    int64_t n_degenerate_faces;   /* nf - nf' */
    int64_t chunk_faces;          /* faces a chunk */
    int64_t chunks_per_group;     /* G */
    int64_t groups;
    int64_t items;                /* (query block, group) work items */
    int64_t n_launches, bytes_uploaded, bytes_downloaded;
    int64_t bytes_scratch;        /* the partial records: nq x groups x 32 */
} mm_winding_report;              /* 80 bytes */

/* Per query i: out_n[i] quarter turns, out_p[2 i], out_p[2 i + 1] = P, out_rho[i], out_touch[i] (0 or 1); without a
 * staged face n = 0, P = (1, 0), rho = +inf, touch = 0.  nf == 0 or nq == 0 is valid.  MM_ERR_INVALID: a non-finite
 * coordinate or one above 2^300 in vertices or queries, a face index out of range, nv, nf or nq of 2^31 or more;
 * MM_ERR_TOO_LARGE: more than 2^31 - 1 work items.  On an error the outputs are not written. */
int     mm_mesh_winding(mm_engine* e, const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf,
                        const double* queries_xyz, int64_t nq, int32_t* out_n, double* out_p, double* out_rho,
                        uint8_t* out_touch, mm_winding_report* report);
/* Rule 8 on the host: out_w and out_err from (n, p, rho, touch) of nq queries and nf' = n_staged. */
int     mm_winding_result(const int32_t* n, const double* p, const double* rho, const uint8_t* touch, int64_t nq,
                          int64_t n_staged, double* out_w, double* out_err);
/* TEST HOOK (no engine, no device): the grouping of rule 7 for n_staged faces.  info[4] = {faces per chunk, G, groups,
 * n_staged}. */
int     mm_winding_plan(int64_t n_staged, int64_t* info);
/* TEST HOOK (no engine, no device): mm_mesh_winding on the host by the arithmetic the kernels run
 * (csrc/mm_winding_device.h), in the same grouping.  *n_staged = nf'. */
int     mm_winding_fold_host(const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf,
                             const double* queries_xyz, int64_t nq, int32_t* out_n, double* out_p, double* out_rho,
                             uint8_t* out_touch, int64_t* n_staged);

/* ---- branch labelling(multimodars/ccta/labeling.py:415-487) -------------------------------------------------------- */

#define MM_BRANCH_MASK_BITS 64   /* branch ids a mask holds: a centerline point with a larger branch_id is MM_ERR_INVALID */

/* masks_out[i] bit b = 1 iff some centerline point with branch_id b lies within squared distance <= radius * radius of
 * point i: the test of mm_centerline_bounded_points (the same operands in the same order, exact f64), so the mask equals
 * one call of that function per branch, bit for bit, from one upload and one launch (mm_branch_kernels.hip).  An empty
 * point set or centerline, like a NULL array, is MM_ERR_INVALID. */
int     mm_branch_masks(mm_engine* e, const mm_clpoint* cl, int64_t ncl, const double* pts_xyz, int64_t n, double radius,
                        uint64_t* masks_out);
/* Centerline points of one LDS tile of that kernel (a longer centerline is staged tile after tile). */
int     mm_branch_tile_points(void);
/* The lists of label_branches from n masks, host only.  MAIN = the bits of main_ids (n_main of them, each below
 * MM_BRANCH_MASK_BITS).  main_idx: the points with mask & MAIN != 0; side_idx: all others; both in input order, capacity
 * n, nullable.  side_k of branch k (0 <= k < n_branches <= MM_BRANCH_MASK_BITS): the side points with bit k, in input
 * order, at side_k_idx[side_k_off[k] .. side_k_off[k + 1]) (side_k_off: n_branches + 1 entries; a main branch's range is
 * empty; a point near several side branches is in each of their lists).  counts[3] = {main, side, all side_k entries};
 * side_k_idx (nullable) is written only where counts[2] <= side_k_cap. */
int     mm_branch_select(const uint64_t* masks, int64_t n, const uint32_t* main_ids, int64_t n_main, int64_t n_branches,
                         int64_t* main_idx, int64_t* side_idx, int64_t* side_k_off, int64_t* side_k_idx, int64_t side_k_cap,
                         int64_t* counts);
/* label_branches (labeling.py:453-487) in one launch: mm_branch_masks into masks_out (n entries), then mm_branch_select
 * on them.  Equal to the reference's sequence of per-branch searches and set differences, duplicated points included:
 * points with equal coordinates have equal masks. */
int     mm_label_branches(mm_engine* e, const mm_clpoint* cl, int64_t ncl, const double* pts_xyz, int64_t n, double radius,
                          const uint32_t* main_ids, int64_t n_main, int64_t n_branches, uint64_t* masks_out,
                          int64_t* main_idx, int64_t* side_idx, int64_t* side_k_off, int64_t* side_k_idx, int64_t side_k_cap,
                          int64_t* counts);

/* ---- B-spline contours (multimodars/ccta/discretization_map.py:16-101) --------------------------------------------- */

/* Most points one contour of mm_bspline_fit_closed_batch may have.  The fit keeps a contour's whole problem in one
 * block's LDS: 39 (m + 10) + 11 m doubles at degree 5, about 102 KB at m = 256, inside the 160 KB a gfx950 block may
 * take. */
#define MM_BSPLINE_MAX_POINTS 256

/* out_status of mm_bspline_fit_closed_batch */
enum mm_bspline_status {
    MM_BSPLINE_FITTED               = 0,  /* |fp - s| <= 1e-3 s (FITPACK ier 0)                                  */
    MM_BSPLINE_INTERPOLATED         = 1,  /* s = 0, or the knots grew to the interpolation set (ier -1)          */
    MM_BSPLINE_COLLAPSED            = 2,  /* the best constant already has fp0 - s < 1e-3 s: one point (ier -2)  */
    MM_BSPLINE_UNCHANGED_SHORT      = 3,  /* fewer than degree + 1 points: returned as it is                     */
    MM_BSPLINE_UNCHANGED_ZERO_CHORD = 4,  /* two consecutive points coincide (ier 10): returned as it is         */
    MM_BSPLINE_UNCHANGED_NONFINITE  = 5,  /* a non-finite coordinate, or a singular system: returned as it is    */
    MM_BSPLINE_ITERATION_LIMIT      = 6   /* the search for p stopped early (ier 1, 2, 3): the result is used    */
};

/* Replace each of n_contours contours (CSR: contour j = points offsets[j] .. offsets[j + 1] of xyz) by m points on its
 * closed smoothing B-spline of the given degree (1..5) and smoothing s >= 0: scipy's splprep(s, k, per=True) followed by
 * splev at u = i / m, restated.  The last point of a contour is replaced by its first before the fit, as
 * splprep does.  out_xyz: as many points as xyz; out_centroid: 3 per contour, np.mean of each output coordinate in
 * numpy's pairwise order; out_status: one mm_bspline_status; out_fp: the residual sum of squares; out_nknots: the knot
 * count (0 for an unchanged contour).  Every contour is fitted in one launch (mm_bspline_kernels.hip), bit for bit the
 * arithmetic of tests/mm_checkers/bspline.py.  A degree outside 1..5, a negative or non-finite smoothing, or a contour of
 * more than MM_BSPLINE_MAX_POINTS points is MM_ERR_INVALID for the whole call, and no output is written; so is
 * MM_ERR_TOO_LARGE on a device whose LDS per block cannot hold the longest contour's system. */
int     mm_bspline_fit_closed_batch(mm_engine* e, int64_t n_contours, const double* xyz, const int64_t* offsets,
                                    double smoothing, int degree, double* out_xyz, double* out_centroid,
                                    int32_t* out_status, double* out_fp, int32_t* out_nknots);
/* MM_BSPLINE_MAX_POINTS */
int     mm_bspline_max_points(void);

#ifdef __cplusplus
}
#endif
#endif
