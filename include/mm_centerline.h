/*
 * mm_centerline.h -- C ABI of the centerline placement path: three-point initial rotation,
 * frame placement on the centerline and the Hausdorff refinement grid (the third call site of
 * the Hausdorff search).  Same conventions as mm_hausdorff.h:
 * plain pointers and sizes, caller-owned arrays updated in place, 0 or a negative MM_ERR_* code,
 * message in mm_last_error().
 *
 * Reference interfaces replaced (paths relative to the reference checkout):
 *   src/types/native/centerline.rs:14-62                         Centerline::from_contour_points,
 *                                                                find_reference_cl_point_idx
 *   src/intravascular/centerline_align/preprocessing.rs:16-108   preprocess_centerline
 *   src/types/native/contour.rs:368-405                          Contour::sort_contour_points
 *   src/types/native/geometry.rs:241-250                         Geometry::rotate_geometry
 *   src/intravascular/centerline_align/align_algorithms.rs:96-126,511-535  apply_transformations
 *   src/intravascular/centerline_align/align_algorithms.rs:263-336         best_rotation_three_point
 *   src/intravascular/centerline_align/align_algorithms.rs:339-451         refine_alignment_hausdorff
 *   src/intravascular/centerline_align/align.rs:63-285           align_three_point_rs, align_manual_rs,
 *                                                                align_combined_rs (write = false)
 * Python entry points that bind them: multimodars/_processing.py:1010-1300
 * (binding src/intravascular/binding/align.rs:83-460).
 *
 * The geometry transforms are host f64 (they are O(points)); every Hausdorff evaluation of the
 * refinement grid runs on the device through the same exact-f64 kernels as mm_hausdorff_batch.
 */
#ifndef MM_CENTERLINE_H
#define MM_CENTERLINE_H

#include "mm_hausdorff.h"

#ifdef __cplusplus
extern "C" {
#endif

/* CenterlinePoint (types/native/centerline_point.rs:4-11), 64 bytes */
typedef struct {
    double   x, y, z;        /* contour_point coordinates */
    double   tx, ty, tz;     /* tangent                   */
    double   radius;
    uint32_t branch_id;      /* 0 = main vessel           */
    uint32_t pad_;
} mm_clpoint;

/* A Geometry as the placement code reads it: mm_geometry plus the lumen contour's own centroid
 * (Contour.centroid, which Frame::rotate leaves stale -- align_frame reads it, :130-135) and the
 * boundaries of the individual extras contours (each is sorted on its own after a rotation). */
typedef struct {
    mm_geometry* g;
    uint8_t*  has_lumen_centroid;  /* [F] Frame.lumen.centroid.is_some(); NULL = all None       */
    double*   lumen_centroid;      /* [F*3]                                                    */
    int32_t   n_extra_kinds;       /* K extras contours per frame inside g->extra (catheter excluded) */
    int64_t*  extra_kind_off;      /* [F*K+1] CSR over (frame, kind) into g->extra; NULL = one contour per frame */
    /* ContourPoint.aortic of the lumen and of the Wall contour (nullable = all false).  A sort moves whole
     * ContourPoints (contour.rs:385-390), so these are permuted with their points by every function here that
     * sorts contours; mm_align_walls reads the wall's (align.rs:385-407). */
    uint8_t*  lumen_aortic;        /* [lumen points]                                                          */
    uint8_t*  wall_aortic;         /* [wall points, frame by frame]                                           */
    int32_t   wall_kind1;          /* 1 + index of the Wall contour among the K kinds; 0 = no Wall contours   */
} mm_cl_geometry;

/* Centerline::from_contour_points (centerline.rs:14-42): tangents = normalised forward
 * differences, last point repeats its predecessor's.  xyz: n triples.  n == 1 is an error (the
 * reference panics). */
int     mm_centerline_from_points(const double* xyz, int64_t n, mm_clpoint* out);
/* find_reference_cl_point_idx (centerline.rs:51-62): first point of minimal 3-D distance. */
int64_t mm_centerline_find_ref_idx(const mm_clpoint* cl, int64_t n, const double ref[3]);
/* preprocess_centerline (preprocessing.rs:16-108): branch 0 only, descending z, resampled at
 * the mean spacing of ref_mesh's frame centroids.  Returns the number of points (writes up to
 * cap of them; call with cap = 0 to size the buffer) or a negative error. */
int64_t mm_centerline_preprocess(const mm_clpoint* cl, int64_t n, const mm_geometry* ref_mesh,
                                 mm_clpoint* out, int64_t cap, double* spacing);

/* ---- branch structure (centerline.rs:64-937), host f64 in the reference's operation order (mm_cl_branches.cpp).
 * A branch is a maximal run of consecutive points with one branch_id (the reference's branch_start_indices are the
 * first indices of those runs); `branch` arguments count runs from 0, which is the branch_id wherever one of these
 * functions has numbered them.  ContourPoint.point_index is the position in the array.  Every function writes a new
 * centerline into out (never the input array) and returns its number of points, or a negative error; branch ids are
 * renumbered 0, 1, ... and tangents recomputed inside branches (recompute_tangents, :377-391) wherever the reference
 * rebuilds, and the input is copied unchanged wherever the reference returns early. */

/* calculate_branches (:78-155): the branches of a centerline whose segments were written one after the other.  Gaps
 * above p95(consecutive spacing) * spacing_tolerance start a segment; segments are joined by one edge at their closest
 * pair where that is within the threshold; the longest path by arc length (double BFS from point 0) becomes branch 0,
 * the remaining components side branches in descending size (ties: discovery order), each walked as a chain; components
 * of fewer than 5 points are dropped.  out holds n points.  A coordinate that is not finite is MM_ERR_INVALID (the
 * reference's sort of the spacings has no defined order then). */
int64_t mm_centerline_calculate_branches(const mm_clpoint* cl, int64_t n, double spacing_tolerance, mm_clpoint* out);
/* find_sharp_angles (:436-466): the positions of the interior points of the branch whose opening angle has
 * cos > cos_threshold (both legs at least 1e-10 long), ascending, into out_idx (capacity n).  An absent branch: 0. */
int64_t mm_centerline_find_sharp_angles(const mm_clpoint* cl, int64_t n, uint32_t branch, double cos_threshold,
                                        int64_t* out_idx);
/* split_branch (:474-505) at position point_index, which both pieces keep; branches re-sorted by descending number of
 * points (stable).  out holds n + 1 points.  An absent branch, a position outside it or at one of its ends: unchanged. */
int64_t mm_centerline_split_branch(const mm_clpoint* cl, int64_t n, uint32_t branch, int64_t point_index, mm_clpoint* out);
/* merge_branches (:512-553): the two branches joined at their closest pair of ends (the first of the four pairings
 * within 1e-12 of the smallest distance, in the order last-first, last-last, first-first, first-last), re-sorted as
 * above.  out holds n points.  Equal or absent branches: unchanged. */
int64_t mm_centerline_merge_branches(const mm_clpoint* cl, int64_t n, uint32_t branch_a, uint32_t branch_b, mm_clpoint* out);
/* orient_by_max_z (:570-587): branch 0 reversed unless its point of largest z (the LAST of equal maxima) is its first;
 * every other branch reversed where its last point is nearer to branch 0 (as it then stands) than its first. */
int64_t mm_centerline_orient_by_max_z(const mm_clpoint* cl, int64_t n, mm_clpoint* out);
/* orient_to_reference (:599-615): every branch reversed where its last point is strictly nearer than its first to the
 * reference's first branch (minimum over its points).  An empty reference reverses nothing. */
int64_t mm_centerline_orient_to_reference(const mm_clpoint* cl, int64_t n, const mm_clpoint* reference, int64_t n_ref,
                                          mm_clpoint* out);
/* remove_branch_overlap (:681-692, 877-913): from every side branch, in order, the leading points within branch 0's mean
 * spacing of a point of branch 0 or of an earlier, already trimmed branch are removed but the last of them (the
 * junction); a branch wholly within is dropped. */
int64_t mm_centerline_remove_branch_overlap(const mm_clpoint* cl, int64_t n, mm_clpoint* out);
/* trim_start (:698-708, 917-937): the first points of branch 0 up to the last whose arc length from the start is
 * <= mm_len are removed; mm_len <= 0: unchanged. */
int64_t mm_centerline_trim_start(const mm_clpoint* cl, int64_t n, double mm_len, mm_clpoint* out);
/* smooth (:798-866): positions replaced by a Gaussian mean over the points with the same branch_id, sigma in points,
 * truncated at ceil(3 sigma) and at the nearer end of the branch on BOTH sides alike; tangents recomputed; branch ids
 * kept.  sigma < 1e-12: unchanged. */
int64_t mm_centerline_smooth(const mm_clpoint* cl, int64_t n, double sigma, mm_clpoint* out);

/* Contour::sort_contour_points (contour.rs:368-405) on n xyz triples, in place. */
int     mm_sort_contour_points(double* xyz, int64_t n);
/* Geometry::rotate_geometry (geometry.rs:241-250): every frame about its own centroid, then
 * every contour re-sorted; angle == 0.0 returns without sorting. */
int     mm_rotate_geometry(mm_cl_geometry* g, double angle);
/* apply_transformations (align_algorithms.rs:511-535 with get_transformations :96-126 and
 * align_frame :128-173): geoms[0] is the primary geometry the transformations are computed from;
 * all n_geoms (1 or 2: Geometry or GeometryPair) receive them.  Returns the number of frames
 * placed (frames past the end of the centerline stay untouched) or a negative error. */
int64_t mm_apply_transformations(mm_cl_geometry** geoms, int n_geoms, const mm_clpoint* cl, int64_t ncl,
                                 const double ref_pt[3]);
/* best_rotation_three_point (align_algorithms.rs:263-336): sweep 0..2pi in accumulated steps of
 * angle_step over the reference frame's lumen (n xyz triples, point_index == position). */
int     mm_best_rotation_three_point(const double* lumen_xyz, int64_t n, int has_centroid,
                                     const double centroid[3], uint32_t index_reference,
                                     const double p_main[3], const double p_ccw[3], const double p_cw[3],
                                     double angle_step, const mm_clpoint* clp, double* best_angle);

/* refine_alignment_hausdorff (align_algorithms.rs:339-451).  The (index shift x angle) grid is
 * rebuilt on the host (rotate + sort + place + downsample per candidate, candidates in
 * parallel), then every candidate's hausdorff_distance(filtered CCTA points, placed frames) is
 * evaluated on the device in one batch; the first minimum in (index asc, angle asc) order wins
 * (strict `<`, :433).  all_costs (nullable, cap entries) receives the evaluated candidates'
 * costs in that order, *n_evals their number. */
int     mm_refine_alignment_hausdorff(mm_engine* e, mm_cl_geometry** geoms, int n_geoms,
                                      const mm_clpoint* cl, int64_t ncl, int64_t initial_cl_ref_idx,
                                      double initial_rotation, const double* points_xyz, int64_t n_points,
                                      double angle_search_range, double angle_step, int64_t index_search_range,
                                      double* best_angle, int64_t* best_idx, double* min_hausdorff,
                                      double* all_costs, int64_t cap, int64_t* n_evals);

/* align_walls (align.rs:381-595): with anomalous != 0 and at least two frames in geoms[0], the Wall contour of every
 * frame (but the first) of every geometry is rotated about its lumen normal so that its aortic side -- or, without
 * aortic flags, its major axis -- follows the direction of frame 0's wall, parallel-transported along the vessel.
 * Lumen and all other contours stay.  The reference holds no test of this function: parity is against
 * oracle/mm_oracle_cl.c's restatement only ("parity unpinned"). */
int     mm_align_walls(mm_cl_geometry** geoms, int n_geoms, int anomalous);

/* align_three_point_rs / align_manual_rs / align_combined_rs (align.rs:63-124, 126-166, 169-285)
 * with write = false.  geoms (1 or 2) are transformed in place; angles in radians except
 * rotation_angle_deg; *total_rotation is in radians (the binding converts, align.rs:125).
 * align_wall_anomalous != 0: mm_align_walls as the last step (align.rs:105-107,147-149,266-268). */
int     mm_align_three_point(const mm_clpoint* cl, int64_t ncl, mm_cl_geometry** geoms, int n_geoms,
                             uint32_t ref_point_index, const double p_main[3], const double p_ccw[3],
                             const double p_cw[3], double angle_step, int align_wall_anomalous,
                             double* spacing, double* total_rotation);
int     mm_align_manual(const mm_clpoint* cl, int64_t ncl, mm_cl_geometry** geoms, int n_geoms,
                        double rotation_angle_deg, const double ref_pt[3], int align_wall_anomalous,
                        double* spacing, double* total_rotation);
int     mm_align_combined(mm_engine* e, const mm_clpoint* cl, int64_t ncl, mm_cl_geometry** geoms, int n_geoms,
                          uint32_t ref_point_index, const double p_main[3], const double p_ccw[3],
                          const double p_cw[3], const double* points_xyz, int64_t n_points,
                          double angle_step, double refine_angle_range, int64_t refine_index_range,
                          int align_wall_anomalous, double* spacing, double* total_rotation,
                          int64_t* refined_idx, int64_t* n_evals);

/* ---- centerline from a mesh: geodesic field, band skeleton, tree (mm_geodesic.cpp, mm_geodesic_kernels.hip; DESIGN
 * 4.26).  The reference has no such function ("Create Centerline directly from mesh" is an open item of its roadmap); the
 * rules are this project's own, restated in tests/mm_checkers/mesh_skeleton.py.  Arguments as the mesh calls of
 * mm_ccta.h: nv, nf, n_seeds below 2^31 and 6 nf below 2^31 (MM_ERR_TOO_LARGE), a face index or a seed outside [0, nv),
 * n_seeds == 0 and a band that is not finite and positive are MM_ERR_INVALID before anything is allocated; nv == 0
 * launches nothing.  Coordinates may be anything: an edge with an end that is not finite is skipped, not refused.
 *
 * Rule G, the field.  The graph is the distinct undirected edges {lo < hi} of the faces; (a, a) is not an edge.  An
 * edge weighs w = sqrt((dx dx + dy dy) + dz dz), d = v[hi] - v[lo] per component, unfused f64, computed once so that
 * both directions see the same bits; an edge whose weight is not finite is left out and counted (n_skipped_edges).
 * dist[s] = +0.0 at the seeds; elsewhere dist[v] is the minimum over the edge paths from any seed of the sum of the
 * weights along the path, rounded after every addition, from the seed on; +inf where no path arrives.  That is what
 * Dijkstra's algorithm returns, and it is the one fixpoint of d[v] = min(d[v], fl(d[u] + w)) below the start, in any
 * order, because the rounded addition of a non-negative weight is monotone: the result has one bit pattern whatever the
 * schedule.  A finite weight is the square root of a finite double and so below 2^512: fewer than 2^31 of them cannot sum
 * to +inf, and every vertex joined to a seed by kept edges is reached.  A mesh whose squared differences all underflow has
 * every weight +0.0, and every vertex reached lies at +0.0.  pred[v] = the smallest neighbour u with fl(dist[u] + w(u, v))
 * == dist[v], -1 at seeds and where dist is +inf (edges of weight zero can make two vertices each other's predecessor).
 * n_edges counts the edges kept,
 * n_reached the vertices with a finite distance (seeds included), max_dist the largest finite distance, max_edge the
 * longest finite weight.  rounds, n_batches and n_launches describe the schedule and are no function of the input
 * alone: a round relaxes every flagged block of 256 consecutive vertices to its local fixpoint, and the host reads the
 * rounds' marks once per batch of 8, 16, 32, then 64 rounds. */
typedef struct {
    int64_t n_vertices, n_faces, n_edges, n_skipped_edges, n_reached, rounds, n_batches, n_launches, bytes_uploaded,
            bytes_downloaded;
    double  max_dist, max_edge;
} mm_geodesic_report;

int     mm_mesh_geodesic(mm_engine* e, const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf,
                         const int64_t* seeds, int64_t n_seeds, double* dist, int64_t* pred, mm_geodesic_report* report);

/* Rule S, the nodes (on the device, mesh and field resident: one upload, one download).  band[v] = (int64)(dist[v] /
 * band_mm) where dist is finite, from one f64 division, -1 elsewhere; a quotient of 2^31 or more is MM_ERR_TOO_LARGE.  A
 * node is a connected component, under the graph's edges, of the vertices of one band; nodes are numbered by (band,
 * smallest vertex) ascending and vertex_node[v] is that number, or -1.  A band narrower than the edges breaks the rings
 * into crumbs: callers take twice the longest edge (the report's field.max_edge) unless they know better.
 *   Sums, area-weighted.  a_f = 0.5 * sqrt((cx cx + cy cy) + cz cz), c = (v1 - v0) x (v2 - v0), c_x = e1_y e2_z - e1_z
 * e2_y and so on; a3 = a_f / 3.  Over the faces in ascending index and in each the corners 0, 1, 2, a corner whose
 * vertex p lies in node n adds a3 to W_n and a3 * p to S_n per component, sequentially, unfused f64; centre = S_n / W_n;
 * radius = (the same sum of a3 * |p - centre|) / W_n; weight = W_n.  A node with a corner whose a3 is not finite, or
 * with W_n not above zero, takes the plain mean of its vertices in ascending index instead (the sum, then one division
 * by their number), radius the plain mean of |p - centre|, weight +0.0, and flag bit 1.  radius_min is the smallest
 * |p - centre| over the node's vertices (a NaN is passed over).  |d| = sqrt((dx dx + dy dy) + dz dz).
 *   flags bit 0: the node holds a rim vertex that is not a seed -- an end of an edge {lo < hi} that exactly one corner
 * of one face spans, as the trimming counts open edges; bit 1: the plain mean was used; bit 2: the node holds a seed.
 *   Node edges: the distinct pairs (lo node < hi node) joined by at least one edge of the graph, sorted.
 * Capacities as mm_mesh_adjacency_csr: where n_nodes > node_cap or n_node_edges > edge_cap the report holds both counts,
 * nothing else is written and MM_ERR_TOO_LARGE returns.  union_rounds, n_launches and the field's schedule numbers are no
 * function of the input alone. */
typedef struct {
    double  x, y, z, radius, radius_min, weight;
    int64_t band, first_vertex, n_vertices, flags;
} mm_skeleton_node;

typedef struct {
    mm_geodesic_report field;
    int64_t n_nodes, n_node_edges, union_rounds, n_launches, bytes_uploaded, bytes_downloaded;
    double  band_mm;
} mm_skeleton_report;

int     mm_mesh_skeleton(mm_engine* e, const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf,
                         const int64_t* seeds, int64_t n_seeds, double band_mm, int64_t node_cap, int64_t edge_cap,
                         double* dist, int64_t* pred, int64_t* vertex_node, mm_skeleton_node* nodes, int64_t* edges,
                         mm_skeleton_report* report);

/* Rule T, terminals, tree, branches (host only, no engine).  nodes in band order (as mm_mesh_skeleton numbers them),
 * edges lo < hi; a terminal is a point behind a node (the node of a rim loop's smallest vertex).
 *   Parent: the adjacent node of lower band with the smallest number; a node with flag bit 2, or without a lower
 * neighbour, is a root.  n_loops = edges - nodes + components, reported, never an error.
 *   Open ends: a node with flag bit 0 is dropped when all its descendants have the bit too (the partial rings before an
 * open outlet, whose centroids walk off to the wall); a root is never dropped; elsewhere the bit means nothing here.
 *   Terminals: terminal j becomes point n_nodes + j, a leaf behind the first kept node on the parent chain from its node.
 *   Paths: the length of a tree edge is |child - parent| = sqrt((dx dx + dy dy) + dz dz), a path's length the sum from its
 * upper end down, left to right.  Roots in ascending number.  A root's first branch is its path to the leaf of greatest
 * length from the root (the smaller number among equals).  Then, repeatedly, of the leaves not yet taken the one whose
 * path down from its first ancestor already in the output (the junction) is longest, the smaller number among equals: it
 * is pruned when that length is below min_branch_mm -- below twice the junction's radius where min_branch_mm is negative --
 * and the leaf is no terminal; else it becomes the next branch, from its first point off the junction to the leaf.
 * Branch ids count from 0 across the roots; the first root's first branch is branch 0, the main vessel.
 *   Output: out (cap >= n_nodes + n_terminals points) with radius = the node's or terminal's, tangents by the rule of
 * recompute_tangents; point_node[i] = the node (or n_nodes + j) of point i; branch_info[4 b ..] = parent branch, the
 * junction's index in out (-1, -1 for a root's first branch), 1 where the branch ends in a terminal, its number of
 * points.  Returns the number of points, or a negative error. */
typedef struct {
    double  x, y, z, radius;
    int64_t node;
} mm_skeleton_terminal;

typedef struct {
    int64_t n_points, n_branches, n_roots, n_components, n_loops, n_dropped_open, n_pruned, n_terminals;
} mm_tree_report;

int64_t mm_skeleton_centerline(const mm_skeleton_node* nodes, int64_t n_nodes, const int64_t* edges, int64_t n_edges,
                               const mm_skeleton_terminal* terminals, int64_t n_terminals, double min_branch_mm,
                               mm_clpoint* out, int64_t* point_node, int64_t* branch_info, int64_t cap,
                               mm_tree_report* report);

#ifdef __cplusplus
}
#endif
#endif
