// mm_device.h -- shared by the HIP kernel files (mm_*_kernels.hip) and the host files that drive them: the search engine's
// structures and every file's launchers; the CCTA point kernels' records are in mm_point_records.h.  Internal.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

#include "mm_point_records.h"
#include "mm_search_records.h"
#include "mm_screen_limits.h"

namespace mm {

// Launchers (mm_kernels.hip).  All asynchronous on `s`.
hipError_t launch_screen_f32(const BatchDev& b, int max_na, int max_nbp, hipStream_t s);
hipError_t launch_screen_fast(const BatchDev& b, int max_na, int max_nbp, hipStream_t s);
// matrix-pipe screen (MM_PRECISION_F32_MATRIX) over the work items [work_begin, work_begin + n_work) of b.work: every one
// of their pairs must have sets of mx_min_points() .. mx_max_points() points, a target set whose variant (mx_variant) is
// (nct, multi), a reference set of at most a_cap row tiles of 32, and PairDesc::pad0 = the pair's scale exponent
hipError_t launch_screen_mx(const BatchDev& b, int work_begin, int n_work, int nct, int multi, int a_cap, hipStream_t s);
// the same screen without the tiles that provably hold no minimum (k_screen_mx_cull): pairs whose variant mx_cull_takes;
// tiles (nullable): device counter of the tiles computed.  runs (nullable, device memory): n_runs runs that hold every one
// of the n_work items once, `first` counted from work_begin, each of one pair -- a workgroup per run, in the table's order;
// without it a workgroup per item
hipError_t launch_screen_mx_cull(const BatchDev& b, int work_begin, int n_work, const WorkRun* runs, int n_runs, int nct, int a_cap,
                                 unsigned long long* tiles, int pair, int floor, hipStream_t s);
hipError_t launch_screen_none(const BatchDev& b, int work_begin, int n_work, hipStream_t s);   // screened value 0 for every candidate
// bounded screen: lower bound of every lb_candidate_step()-th candidate -> per-pair pick -> full screen of
// the picks (upper bound) -> spread the bounds to the candidates in between (chord inequality) ->
// lower bound of those still possible -> survivors -> full screen of the survivors (runs of <= 8
// candidates, at most `cap` of them)
hipError_t launch_screen_lb(const BatchDev& b, int max_nap, int max_nbp, hipStream_t s);
hipError_t launch_lb_pick(const BatchDev& b, int round, hipStream_t s);
hipError_t launch_screen_picks(const BatchDev& b, int round, int max_na, int max_nbp, hipStream_t s);
hipError_t launch_lb_spread(const BatchDev& b, hipStream_t s);
hipError_t launch_screen_lb_queued(const BatchDev& b, int max_nap, int max_nbp, int cap, hipStream_t s);
hipError_t launch_lb_keep(const BatchDev& b, int final, int cap, hipStream_t s);
// round 3: the pick's decisive points (largest row / column minima) as queries for the survivors
hipError_t launch_lb_topk(const BatchDev& b, int max_n, hipStream_t s);
hipError_t launch_screen_lb_list(const BatchDev& b, int max_nap, int max_nbp, int cap, hipStream_t s);
hipError_t launch_screen_kept(const BatchDev& b, int max_na, int max_nbp, int cap, hipStream_t s);
// large-set Hausdorff (no LDS limit on the set sizes); pairs/work are device arrays of the kernel's
// LargePair {a_off, na, b_off, nb, col_off, pad} / LargeWork {pair, row0} records
hipError_t launch_hausdorff_large(const void* pairs, const void* work, int n_pairs, int n_work, const double* px,
                                  const double* py, void* colmin, long long n_col, void* rowmax, double* out,
                                  hipStream_t s);
// lower bounds of the same pairs: two directed entries per output slot (a->b and b->a; col_off = slot,
// pad = subset stride), out[slot] <= the pair's Hausdorff distance, computed from the same d^2 bits
hipError_t launch_hausdorff_large_bound(const void* pairs, const void* work, int n_out, int n_work, const double* px,
                                        const double* py, void* rowmax, double* out, hipStream_t s);
int        large_rows_per_block();
// 3-D nearest-neighbour squared distances (mm_nn_kernels.hip); pairs / work are device arrays:
// work_a always runs, work_b items first check their bound against their queries' current minima
hipError_t launch_nn3_min(const NnPair* pairs, const NnWork* work_a, int n_a, const NnWork* work_b, int n_b,
                          const double* px, const double* py, const double* pz, const int32_t* qperm, double* out,
                          long long n_out, hipStream_t s);
// neighbour counts within a radius (same records; every work item runs): out[n_out] u32
hipError_t launch_nn3_count(const NnPair* pairs, const NnWork* work, int n_work, const double* px, const double* py,
                            const double* pz, const int32_t* qperm, double r2, unsigned int* out, long long n_out,
                            hipStream_t s);
// derived sets: base point + unit vector * adj where flagged, from 7 planes of n_aux doubles (bx by bz ux uy uz flag),
// written into the SoA point pool
hipError_t launch_nn3_morph(const NnMorph* items, int n_items, const double* aux, long long n_aux, double* px, double* py,
                            double* pz, hipStream_t s);
// sums[p] = the minima of pair p added up in index order (sequential f64 fold)
hipError_t launch_nn3_sums(const NnPair* pairs, int n_pairs, const double* out, double* sums, hipStream_t s);
int        nn_queries_per_block();
int        nn_chunk_points();
int        nn_span_chunks();
// point-to-triangle distances (mm_tri_kernels.hip).  tri12: nf staged faces of 12 doubles (a, b, c as x y z w; a.w = the
// bits of the face's kind, b.w = those of the original face index); qxyz: nq staged queries; work: n_a items of pass
// A, then n_b of pass B.  sq: the minima's bits; key: original face << 32 | staged face of the winner (~0: none); closest:
// 3 per query; region: one; counters[0] = items pass B skipped.  All outputs per query in staged order.
hipError_t launch_tri_distance(const TriWork* work, int n_a, int n_b, const double* tri12, int nf, const double* qxyz, int nq,
                               unsigned long long* sq, unsigned long long* key, double* closest, int32_t* region,
                               unsigned long long* counters, hipStream_t s);
int        tri_launches(int n_b);
// the same over minima seeded with the d2 to one face each (sq) and key = ~0: all n_work items checked, the who pass,
// the closest points; counters[0] += the items skipped
hipError_t launch_tri_seeded(const TriWork* work, int n_work, const double* tri12, int nf, const double* qxyz, int nq,
                             unsigned long long* sq, unsigned long long* key, double* closest, int32_t* region,
                             unsigned long long* counters, hipStream_t s);
int        tri_seeded_launches();
int        tri_queries_per_block();
int        tri_chunk_faces();
// mesh intersections (mm_intersect_kernels.hip; the rule: include/mm_ccta.h, "mesh intersections").  tri12: the staged
// faces, 12 doubles each (a, b, c as x y z w; a.w = canonical id of a | that of b << 32, b.w = that of c | original face
// index << 32, c.w = 1 where the face is degenerate): n_a faces of the first mesh, then n_b of the second from record
// off_b; the self form passes self_form with n_b = n_a, off_b = 0.  items: n_items chunk pairs (I of the first, J of the
// second).  state: one byte per staged record (bit 0 intersecting, bit 1 undecided), n_state_words words; counters[8]:
// intersecting pairs, undecided pairs, coincident pairs, narrow tests, pairs found; pairs: the first `cap` found, as
// state << 62 | first original index << 31 | second.  The clear of state and counters is the first launch.
hipError_t launch_isect_pairs(const int32_t* items, int n_items, const double* tri12, int n_a, int n_b, int off_b,
                              bool self_form, unsigned int* state, long long n_state_words, unsigned long long* counters,
                              unsigned long long* pairs, unsigned long long cap, hipStream_t s);
int        isect_launches();
int        isect_chunk_faces();
// mesh cross-sections (mm_section_kernels.hip; the arithmetic is mm_section_device.h): tri12 = n_faces staged records of
// 12 doubles in slab order (a, b, c as x y z w; a.w = index 0 | index 1 << 32, b.w = index 2 | original face << 32,
// c.w = 1 for a face with a repeated index); planes = 6 doubles each (origin, normal); items = 4 int32 each (chunk,
// first entry of its run in plane_list, planes of the run (at most 64), 0).  counters[8]: [0] = the segments found;
// segments: the first `cap` of them, 72-byte records (section::Segment), in no order.  The clear of the counters is the
// first launch.
hipError_t launch_section_cut(const int32_t* items, int n_items, const int32_t* plane_list, const double* planes,
                              const double* tri12, int n_faces, unsigned long long* counters, void* segments,
                              unsigned long long cap, hipStream_t s);
int        section_launches();
// mesh clipping (mm_clip_kernels.hip; the per-face step is mm_clip_device.h): v, face (int32), rec (nr clip::Record of 48
// bytes, one a cut face), newv (n_new new vertices, new_cut their cuts) and cuts stay resident.  clip_unions: link, the
// marks, frec, counts[clip_num_counts] and status[n_cuts] initialised, the records scattered, the PLANE sides, the unions
// (launch_weld_jump flattens link afterwards).  clip_verdict, links flat: status |= kClipNotSeparating, the drop marks.
// clip_orphan, after a verdict that left every status zero: status |= kClipKeptSideDropped where a kept-side vertex of a
// cut face is dropped.
// clip_counts: vkeep and its scan (vidx, vtile: clip_scan_tiles(nv) + 1 entries, the last the kept vertices), the pieces
// of every face and their scan (foff, ftile likewise, the last the kept faces and pieces).  clip_emit: the result; kv =
// the kept vertices, first_ext / first_cap = where the extension and the cap faces start.  nv > 0 in all of them.
struct ClipCut { double o[3], n[3]; int32_t keep, scope; int32_t pad[2]; };   // 64 bytes
static_assert(sizeof(ClipCut) == 64, "a clip cut is 64 bytes");
enum { clip_num_dropped_faces = 0, clip_num_untouched = 1, clip_num_null_pieces = 2, clip_num_counts = 8 };
enum { kClipScopePlane = 1, kClipNotSeparating = 3, kClipKeptSideDropped = 4 };
enum { kClipUntouched = 0, kClipPiece = 1, kClipExtension = 2, kClipCap = 3 };
hipError_t launch_clip_unions(const double* v, long long nv, const int32_t* face, long long nf, const void* rec, long long nr,
                              const ClipCut* cuts, int n_cuts, unsigned int* link, uint8_t* mark, uint8_t* vdrop, int32_t* frec,
                              unsigned long long* counts, int32_t* status, int* launches, hipStream_t s);
hipError_t launch_clip_verdict(const int32_t* face, const void* rec, long long nr, const unsigned int* link, uint8_t* mark,
                               int32_t* status, int* launches, hipStream_t s);
hipError_t launch_clip_orphan(const int32_t* face, const void* rec, long long nr, const unsigned int* link, const uint8_t* mark,
                              const uint8_t* vdrop, int32_t* status, int* launches, hipStream_t s);
size_t     clip_scan_tiles(long long n);
hipError_t launch_clip_counts(const double* v, long long nv, const double* newv, const int32_t* face, long long nf, const int32_t* frec,
                              const void* rec, const unsigned int* link, const uint8_t* mark, const uint8_t* vdrop, uint8_t* vkeep,
                              int32_t* vidx, long long* vtile, uint8_t* fcnt, int32_t* foff, long long* ftile,
                              unsigned long long* counts, int* launches, hipStream_t s);
hipError_t launch_clip_emit(const double* v, long long nv, const double* newv, const int32_t* new_cut, long long n_new,
                            const int32_t* face, long long nf, const int32_t* frec, const void* rec, long long nr, const int32_t* vidx,
                            long long kv, const uint8_t* fcnt, const int32_t* foff, int layers, int with_cap, long long first_ext,
                            long long first_cap, double* out_v, int32_t* vorigin, int32_t* out_f, int32_t* forigin, uint8_t* fkind,
                            unsigned long long* counts, int* launches, hipStream_t s);
// winding numbers (mm_winding_kernels.hip; the arithmetic is mm_winding_device.h): tri9 = nf staged faces of 9 doubles
// (a, b, c as x y z) in the caller's order, degenerate ones removed; a group is chunks_per_group chunks of
// wind_chunk_faces() faces, none of the `groups` (at most wind_max_groups()) empty.  partials: nq x groups records of 32
// bytes, device scratch, every one written before it is read.  Per query: n quarter turns, p = (pr, pi), rho, touch.
hipError_t launch_winding(const double* tri9, int nf, int chunks_per_group, int groups, const double* qxyz, int nq,
                          void* partials, int32_t* out_n, double* out_p, double* out_rho, int32_t* out_touch, hipStream_t s);
int        wind_launches();
int        wind_queries_per_block();
int        wind_chunk_faces();
int        wind_max_groups();
// ray casting of the occlusion removal (mm_ray_kernels.hip): ray = 6 planes of n_rays doubles (origin xyz, direction
// xyz), tri = 9 planes of n_faces doubles (v0 xyz, e1 = v1 - v0, e2 = v2 - v0); part = n_rays x ceil(n_faces /
// ray_chunk_faces()) records of scratch; closest[r] = the face of ray r's smallest (t, index) if it hits at least 3
// faces, else -1
hipError_t launch_ray_tri(const double* ray, int n_rays, const double* tri, int n_faces, RayPartial* part,
                          int32_t* closest, hipStream_t s);
int        ray_chunk_faces();
int        ray_block_rays();
// nearest slice anchor and plane projection of the vessel discretisation (mm_slice_kernels.hip): jobs = point / anchor
// ranges, work = blocks of slice_block_points() points; pts = xyz triples, anc = 6 doubles per anchor (position, unit
// normal); idx / proj at the point's position
hipError_t launch_slice_nearest(const SliceJob* jobs, const PointWork* work, int n_work, const double* pts,
                                const double* anc, int32_t* idx, double* proj, hipStream_t s);
int        slice_block_points();
// radial morphing about the nearest centerline point (mm_morph_kernels.hip): jobs = point / centerline ranges and the
// adjustment, work = blocks of morph_block_points() points; pts / cl = xyz triples; nearest (job-local centerline
// index) / out (moved xyz) at the point's position
hipError_t launch_cl_morph(const MorphJob* jobs, const PointWork* work, int n_work, const double* pts, const double* cl,
                           int32_t* nearest, double* out, hipStream_t s);
int        morph_block_points();
// lumen morphometry (mm_shape_kernels.hip): one job per contour; xyz = point rows; theta = one angle per point, read
// only when want2d; val = 5 doubles per contour (area, major, minor 3-D, minor 2-D, elliptic ratio), idx = 6 per
// contour (the three pairs, contour-local)
hipError_t launch_contour_measures(const ShapeJob* jobs, int n_jobs, const double* xyz, const double* theta, int want2d,
                                   double* val, int64_t* idx, hipStream_t s);
// mesh trimming (mm_trim_kernels.hip): face = int32 triples, masks uint8 0 / 1.  trim_faces: fkeep per face (all corners
// in `in`, or with any_mode some corner) and the corner marks (nullable); trim_open_edges: the edge keys (min << 32 | max)
// used by exactly one kept face into out (capacity 3 nf), their number in *n_out, through a table of 2^log2_cap slots
// (keys 8 B + counts 4 B each, cleared here; at least twice the insertions); trim_scan: idx[i] = exclusive prefix of the
// nonzero flags (-1 at a zero), tile_sum (trim_scan_tiles(n) + 1 entries) ends with the total; trim_compact: the kept
// vertices gathered and the kept faces remapped; trim_clear: mask[idx[i]] = 0
hipError_t launch_trim_faces(const int32_t* face, long long nf, const uint8_t* in, int any_mode, uint8_t* fkeep,
                             uint8_t* mark, hipStream_t s);
hipError_t launch_trim_open_edges(const int32_t* face, long long nf, const uint8_t* fkeep, unsigned long long* keys,
                                  unsigned int* cnt, int log2_cap, unsigned long long* out, unsigned long long* n_out,
                                  hipStream_t s);
size_t     trim_scan_tiles(long long n);
hipError_t launch_trim_scan(const uint8_t* flag, long long n, long long* tile_sum, int32_t* idx, hipStream_t s);
hipError_t launch_trim_compact(const double* v, long long nv, const int32_t* vidx, const int32_t* face, long long nf,
                               const int32_t* fidx, double* out_v, int32_t* out_f, hipStream_t s);
hipError_t launch_trim_clear(const int32_t* idx, long long n, uint8_t* mask, hipStream_t s);
// mesh assembly (mm_weld_kernels.hip): face = int32 triples.  weld_vertices: rep[v] = the smallest vertex with v's key
// (v itself without a key, -1 unreferenced) through an int32 table of 2^log2_cap slots (at least twice nv), keep[v] =
// rep[v] == v, counts[0] += unreferenced; weld_faces: vmap[v] = vidx[rep[v]] (vidx: the scan of keep), the faces read through it, fkeep = neither
// degenerate nor a later repeat of a vertex set (table: at least twice nf), counts[0..1] += degenerate, repeated;
// weld_edges: the edge table (keys 8 B, counts 4 B, two owners 8 B a slot; at least 6 nf slots, never fewer than 256);
// weld_hook: link = parity union-find over the edges owned twice; weld_jump: one pointer-jumping round, *changed set
// where a link moved; weld_flip: the faces of odd parity reversed, *n_flipped += their number; weld_edge_report:
// counts[0..2] += open, non-manifold, conflicting edges (link nullable: no flips); weld_volume: *out = the adjacent-pair
// tree of the per-face terms (a: nf doubles, b: weld_sum_scratch(nf)); weld_reverse: every face reversed
hipError_t launch_weld_vertices(const double* v, long long nv, const int32_t* face, long long nf, double scale,
                                uint8_t* ref, int32_t* table, int log2_cap, int32_t* rep, uint8_t* keep,
                                unsigned long long* counts, hipStream_t s);
hipError_t launch_weld_faces(const int32_t* face, long long nf, long long nv, const int32_t* rep, const int32_t* vidx,
                             int32_t* vmap, int32_t* table, int log2_cap, int32_t* frep, uint8_t* fkeep,
                             unsigned long long* counts, hipStream_t s);
hipError_t launch_weld_edges(const int32_t* face, long long nf, unsigned long long* keys, unsigned int* cnt,
                             unsigned int* own, int log2_cap, hipStream_t s);
hipError_t launch_weld_hook(const unsigned long long* keys, const unsigned int* cnt, const unsigned int* own,
                            int log2_cap, unsigned int* link, long long nf, hipStream_t s);
hipError_t launch_weld_jump(unsigned int* link, long long nf, unsigned int* changed, hipStream_t s);
hipError_t launch_weld_flip(int32_t* face, long long nf, const unsigned int* link, unsigned long long* n_flipped,
                            hipStream_t s);
hipError_t launch_weld_edge_report(const unsigned long long* keys, const unsigned int* cnt, const unsigned int* own,
                                   int log2_cap, const unsigned int* link, unsigned long long* counts, hipStream_t s);
size_t     weld_sum_scratch(long long nf);
int        weld_volume_launches(long long nf);   // the kernels launch_weld_volume launches for nf faces
hipError_t launch_weld_volume(const double* v, const int32_t* face, long long nf, double* a, double* b, double* out,
                              hipStream_t s);
hipError_t launch_weld_reverse(int32_t* face, long long nf, hipStream_t s);
// mesh closing (mm_close_kernels.hip).  close_half_edges: the edges of weld_edges' table owned by one face, as that face
// traverses them (link nullable: the flips of the winding stage), packed a << 32 | b into out in no fixed order, their
// number in *n_out (cleared here); close_fan: face[nf + i] = (fan[3i+1], fan[3i], nv + fan[3i+2]); smooth_faces: one
// iteration of the label smoothing over the faces (vote: nv words, zero before the first iteration and after every
// one), next = the new labels, *n_flips += the changes, *launches += the kernels launched; smooth_csr: the same over
// the rows of a CSR adjacency
hipError_t launch_close_half_edges(const unsigned long long* keys, const unsigned int* cnt, const unsigned int* own,
                                   int log2_cap, const unsigned int* link, unsigned long long* out,
                                   unsigned long long out_cap, unsigned long long* n_out, hipStream_t s);
hipError_t launch_close_fan(const int32_t* fan, long long n_fan, long long nv, int32_t* face, long long nf, hipStream_t s);
hipError_t launch_smooth_faces(const int32_t* face, long long nf, long long nv, const uint8_t* cur, unsigned int* vote,
                               uint8_t* next, unsigned long long* n_flips, int* launches, hipStream_t s);
hipError_t launch_smooth_csr(const int32_t* off, const int32_t* nb, long long nv, const uint8_t* cur, uint8_t* next,
                             unsigned long long* n_flips, int* launches, hipStream_t s);
// mesh smoothing (mm_smooth_kernels.hip).  Every launcher adds the kernels it launched to *launches.  mesh_csr: from
// weld_edges' table (keys) the sorted adjacency off (nv + 1), nb (as many entries as off[nv]: twice the edges between
// different vertices, at most 6 nf); deg (nv words) and tile_sum (mesh_csr_tiles(nv) + 1) are scratch; counts[0..2] =
// those edges, the vertices without a neighbour, the longest row.  mesh_step: out = one step with factor f over in (two
// buffers of nv xyz triples; pinned nullable).  mesh_ring_seed: ring = -1 everywhere, 0 at the seeds, *reached = the
// distinct seeds; mesh_ring: ring r >= 1 of the level-synchronous search, *reached += the vertices it set.  mesh_disp:
// *max_bits = the bits of the largest squared distance between a and b
size_t     mesh_csr_tiles(long long nv);
// the two halves of mesh_csr that do not read the table, for any rows: row_offsets: off (n + 1) = the exclusive scan of
// the n row lengths in deg, which become the rows' fill cursors, counts[1] += the empty rows, counts[2] = max(counts[2],
// the longest), n >= 1 (3 kernels); row_sort: every row of nb ascending (its entries are distinct; 1 kernel)
hipError_t launch_mesh_row_offsets(int32_t* deg, long long n, int32_t* off, long long* tile_sum, unsigned long long* counts,
                                   int* launches, hipStream_t s);
hipError_t launch_mesh_row_sort(const int32_t* off, int32_t* nb, long long n, int* launches, hipStream_t s);
hipError_t launch_mesh_csr(const unsigned long long* keys, int log2_cap, long long nv, int32_t* deg, int32_t* off,
                           long long* tile_sum, int32_t* nb, unsigned long long* counts, int* launches, hipStream_t s);
hipError_t launch_mesh_step(const int32_t* off, const int32_t* nb, const double* in, double* out, long long nv, double f,
                            const uint8_t* pinned, int* launches, hipStream_t s);
hipError_t launch_mesh_ring_seed(const int32_t* seeds, long long n, int32_t* ring, long long nv,
                                 unsigned long long* reached, int* launches, hipStream_t s);
hipError_t launch_mesh_ring(const int32_t* off, const int32_t* nb, long long nv, int32_t* ring, int32_t r,
                            unsigned long long* reached, int* launches, hipStream_t s);
hipError_t launch_mesh_disp(const double* a, const double* b, long long nv, unsigned long long* max_bits, int* launches,
                            hipStream_t s);
// mesh relaxation (mm_relax_kernels.hip; include/mm_ccta.h, "mesh relaxation").  Queries are the free vertices in staged
// order (qv: their vertex), blocks of tri_queries_per_block(); x: the nv current positions; fkey: each query's face as
// k_tri_min's key (original << 32 | staged, ~0: none); state: nonzero = not moved this iteration; num: the numbers block
// (relax_num_* words).  relax_accept: step 0 -- x, fkey from closest / key, vq[qv[j]] = j (vq: -1 before), the largest
// d2.  relax_candidates: per query block the candidates (qxyz), their seeds (sq, key = ~0), state, the block's box and
// the refreshed lb2 of the block's items (work: n_a items of pass A, then n_b of pass B, as build_plan lays them out;
// cbox: six doubles a chunk).  relax_guard: state |= 2 at the free corners of the faces an iteration would flip.
// relax_apply: x, fkey from closest / key where state == 0; num[reverted] += the others.  relax_flipped:
// num[flipped] += the faces whose normal turned against v0's.
enum { relax_num_vol_before = 0, relax_num_vol_after, relax_num_disp, relax_num_init, relax_num_skipped,
       relax_num_reverted, relax_num_flipped, relax_num_skipped0, relax_num_csr, relax_num_words = relax_num_csr + 4 };
hipError_t launch_relax_accept(const int32_t* qv, int nq, const double* closest, const unsigned long long* key,
                               const unsigned long long* sq, double* x, unsigned long long* fkey, int32_t* vq,
                               unsigned long long* num, hipStream_t s);
hipError_t launch_relax_candidates(const int32_t* off, const int32_t* nb, const double* x, const int32_t* qv, int nq,
                                   const unsigned long long* fkey, const double* tri12, double lambda, double* qxyz,
                                   unsigned long long* sq, unsigned long long* key, unsigned int* state, TriWork* work,
                                   int n_a, int n_b, const double* cbox, hipStream_t s);
hipError_t launch_relax_guard(const int32_t* face, long long nf, const double* x, const double* closest,
                              const unsigned long long* key, const int32_t* vq, unsigned int* state, hipStream_t s);
hipError_t launch_relax_apply(const int32_t* qv, int nq, const double* closest, const unsigned long long* key,
                              const unsigned int* state, double* x, unsigned long long* fkey, unsigned long long* num,
                              hipStream_t s);
hipError_t launch_relax_flipped(const int32_t* face, long long nf, const double* v0, const double* x,
                                unsigned long long* num, hipStream_t s);
// mesh refinement (mm_refine_kernels.hip): face = int32 triples, the edge table as weld_edges sizes it.  refine_edges:
// the table with own[2 s] = the smallest corner id 3 f + j of the slot's edge, slot[3 f + j] = the slot of corner j;
// refine_marks: own[2 s + 1] = 0 where the edge is marked (longer than thr2; with `all` every edge between different
// vertices), ~0 where not; counts (refine_counters() words, cleared here) [0..4] = edges between different vertices,
// open, non-manifold, the bits of the longest squared length, marked; refine_counts: code (nf bytes), tile_sum
// (refine_tiles(nf) entries) -> exclusive packed offsets, counts[5..7] += faces with 1, 2, 3 marked corners, counts[8..9]
// = new vertices, children; refine_offsets: foff[f] = the first child of f, the midpoints nv, nv + 1 ... into v_out,
// their parents into par at (id - nv0), own[2 s + 1] = the midpoint's vertex; refine_edge_list: the marked edges and
// their squared lengths in order instead; refine_children: out = the children (v: the coordinates with the midpoints)
size_t     refine_tiles(long long nf);
int        refine_counters();
hipError_t launch_refine_edges(const int32_t* face, long long nf, unsigned long long* keys, unsigned int* cnt,
                               unsigned int* own, int log2_cap, unsigned int* slot, hipStream_t s);
hipError_t launch_refine_marks(const unsigned long long* keys, const unsigned int* cnt, unsigned int* own, int log2_cap,
                               const double* v, double thr2, int all, unsigned long long* counts, hipStream_t s);
hipError_t launch_refine_counts(const unsigned int* slot, const unsigned int* own, long long nf, uint8_t* code,
                                long long* tile_sum, unsigned long long* counts, hipStream_t s);
hipError_t launch_refine_offsets(const uint8_t* code, long long nf, const long long* tile_off, const unsigned int* slot,
                                 const unsigned long long* keys, unsigned int* own, const double* v, long long nv,
                                 long long nv0, int32_t* foff, double* v_out, int32_t* par, hipStream_t s);
hipError_t launch_refine_edge_list(const uint8_t* code, long long nf, const long long* tile_off, const unsigned int* slot,
                                   const unsigned long long* keys, const double* v, int32_t* edges, double* len_sq,
                                   hipStream_t s);
hipError_t launch_refine_children(const int32_t* face, long long nf, const uint8_t* code, const int32_t* foff,
                                  const unsigned int* slot, const unsigned int* own, const double* v, int32_t* out,
                                  hipStream_t s);
// mesh edge flips (mm_flip_kernels.hip; include/mm_ccta.h, "mesh edge flips"): face = int32 triples, rewritten in place;
// the edge table as weld_edges sizes it, with first (4 bytes a slot) beside it; vw: one word a vertex, deg in the low 31
// bits, the border flag in bit 31; counts: the flip_num_* words, the first flip_num_pass cleared by flip_valence.
// flip_valence: the table, vw and counts[edges .. deviation] of the faces as they are (3 kernels).  flip_pass, behind it:
// prio (8 bytes a slot) and opp (the two opposite corners, 8 bytes a slot) of the candidates, best (8 bytes a vertex),
// counts[candidates .. quality]; then the flips, counts[flips] (2 kernels).  cc2, qk2: the squares of crease_cos and
// quality_keep.
enum { flip_num_edges = 0, flip_num_open, flip_num_nonmanifold, flip_num_inconsistent, flip_num_masked, flip_num_deviation,
       flip_num_candidates, flip_num_existing, flip_num_normal, flip_num_crease, flip_num_quality, flip_num_flips,
       flip_num_pass, flip_num_vol_before = 14, flip_num_vol_after, flip_num_words };
hipError_t launch_flip_valence(const int32_t* face, long long nf, long long nv, const uint8_t* pin,
                               unsigned long long* keys, unsigned int* cnt, unsigned int* own, unsigned int* first,
                               int log2_cap, unsigned int* vw, unsigned long long* counts, hipStream_t s);
hipError_t launch_flip_pass(int32_t* face, long long nv, const double* v, const uint8_t* pin, const unsigned long long* keys,
                            const unsigned int* cnt, const unsigned int* own, const unsigned int* first, int log2_cap,
                            const unsigned int* vw, double cc2, double qk2, unsigned long long* prio, int32_t* opp,
                            unsigned long long* best, unsigned long long* counts, hipStream_t s);
// mesh edge collapse (mm_collapse_kernels.hip; include/mm_ccta.h, "mesh edge collapse"): face = int32 triples, rewritten
// in place; fkeep / vkeep: one byte a face / vertex, 0 once dead; the edge table as weld_edges sizes it, with first beside
// it, of the live faces only; vw: one word a vertex, deg in the low 30 bits, bit 30 = ends an inconsistent edge, bit 31 =
// border; counts: the col_num_* words, the first col_num_pass cleared by col_table.  col_table: the table, vw,
// counts[edges .. short] and prio[s] = 1 at a short edge with two owners of opposite directions, 2 at any other short
// edge, else 0 (2 kernels).  col_pass, behind it and behind launch_mesh_csr on the same keys (off, nb): prio (8
// bytes a slot) and rk (the removed and the kept end, 8 bytes a slot) of the candidates, best (8 bytes a vertex),
// counts[candidates .. quality]; then the collapses, to[r] = k (to: -1 before), counts[collapses] (2 kernels).
// col_finish: target[v] = vidx of the survivor v ended in, origin[vidx[v]] = v (vidx: launch_trim_scan of vkeep).
enum { col_num_edges = 0, col_num_open, col_num_nonmanifold, col_num_inconsistent, col_num_short, col_num_candidates,
       col_num_fixed, col_num_link, col_num_valence, col_num_long, col_num_normal, col_num_quality, col_num_collapses,
       col_num_pass, col_num_vol_before = 14, col_num_vol_after, col_num_words };
hipError_t launch_col_table(const int32_t* face, long long nf, const uint8_t* fkeep, long long nv, const double* v,
                            double thr_min2, unsigned long long* keys, unsigned int* cnt, unsigned int* own,
                            unsigned int* first, int log2_cap, unsigned int* vw, unsigned long long* prio,
                            unsigned long long* counts, hipStream_t s);
hipError_t launch_col_pass(int32_t* face, long long nv, const double* v, const uint8_t* pin, const unsigned long long* keys,
                           const unsigned int* own, const unsigned int* first, int log2_cap, const unsigned int* vw,
                           const int32_t* off, const int32_t* nb, double thr_max2, double cc2, double qk2, unsigned long long* prio, int32_t* rk, unsigned long long* best,
                           uint8_t* fkeep, uint8_t* vkeep, int32_t* to, unsigned long long* counts, hipStream_t s);
hipError_t launch_col_finish(const int32_t* to, const int32_t* vidx, long long nv, int32_t* origin, int32_t* target,
                             hipStream_t s);
// mesh repair (mm_repair_kernels.hip; include/mm_ccta.h, "mesh repair"): face = the input's int32 triples, never written;
// rep[i] = the name a vertex goes by between the stages (the first vertex with its coordinates, or i); wf = the faces
// through rep; fkeep: one byte a face, 0 once dead; counts: the rep_num_* words, cleared by the host.  rep_vertices: rep
// through an int32 table (at least 2 nv slots), counts[welded] (2 kernels).  rep_faces: wf, qb (the bits of q), frep,
// fkeep through an int32 table (at least 2 nf slots), counts[degenerate .. copies] (2 kernels).  rep_edges: the edge
// table of the live faces as weld_edges sizes it, with owners, and eslot[3 f + k] = the slot of the edge leaving corner k
// (1 kernel).  rep_remove, behind it: m1q, m2q (8 bytes a slot), m1f, m2f (4 bytes a slot) = the two largest keys (q,
// face) of every slot with more than two owners; with `act` the faces that are neither die, counts[removed]; link[c] =
// c << 1 for all 3 nf corners (5 kernels).  rep_hook, behind rep_edges of the faces left: the corner sets (1 kernel;
// launch_weld_jump over 3 nf links flattens them).  rep_split: vmin, wmin, wmax (4 bytes a vertex), ref, vsplit, vback,
// vkeep (a byte a vertex), mixed, isnew, cback (a byte a corner), counts[unreferenced .. unwelded] (3 kernels).  rep_output: vidx, fidx, cidx are
// launch_trim_scan of vkeep, fkeep, isnew; kv = the vertices kept; out_v and origin hold kv + the new vertices (2 kernels).
enum { rep_num_welded = 0, rep_num_degenerate, rep_num_null, rep_num_copies, rep_num_edges_before,
       rep_num_edges_after = rep_num_edges_before + 3, rep_num_removed = rep_num_edges_after + 3, rep_num_unreferenced,
       rep_num_split, rep_num_unwelded, rep_num_words = 16 };
hipError_t launch_rep_vertices(const double* v, long long nv, int weld, int32_t* table, int log2_cap, int32_t* rep,
                               unsigned long long* counts, hipStream_t s);
hipError_t launch_rep_faces(const int32_t* face, long long nf, const int32_t* rep, const double* v, int drop_null,
                            int drop_copies, int32_t* table, int log2_cap, int32_t* wf, unsigned long long* qb,
                            int32_t* frep, uint8_t* fkeep, unsigned long long* counts, hipStream_t s);
hipError_t launch_rep_edges(const int32_t* wf, long long nf, const uint8_t* fkeep, unsigned long long* keys,
                            unsigned int* cnt, unsigned int* own, int log2_cap, unsigned int* eslot, hipStream_t s);
hipError_t launch_rep_remove(long long nf, uint8_t* fkeep, const unsigned int* eslot, const unsigned int* cnt,
                             const unsigned long long* qb, int log2_cap, int act, unsigned long long* m1q, int32_t* m1f,
                             unsigned long long* m2q, int32_t* m2f, unsigned int* link, unsigned long long* counts,
                             hipStream_t s);
hipError_t launch_rep_hook(const unsigned long long* keys, const unsigned int* cnt, const unsigned int* own, int log2_cap,
                           const int32_t* wf, unsigned int* link, hipStream_t s);
hipError_t launch_rep_split(long long nf, long long nv, const uint8_t* fkeep, const int32_t* face, const int32_t* wf,
                            const unsigned int* link, const int32_t* rep, int split, int drop, unsigned int* vmin,
                            unsigned int* wmin, unsigned int* wmax, uint8_t* ref, uint8_t* vsplit, uint8_t* vback,
                            uint8_t* mixed, uint8_t* isnew, uint8_t* cback, uint8_t* vkeep, unsigned long long* counts,
                            hipStream_t s);
hipError_t launch_rep_output(const double* v, long long nv, const int32_t* rep, const int32_t* vidx, long long nf,
                             const uint8_t* fkeep, const int32_t* fidx, const int32_t* face, const int32_t* wf,
                             const unsigned int* link, const uint8_t* cback, const int32_t* cidx, long long kv, double* out_v, int32_t* out_f, int32_t* origin,
                             int32_t* target, hipStream_t s);
// geodesic field (mm_geodesic_kernels.hip; include/mm_centerline.h, "Rule G"): off, nb = the sorted adjacency of
// launch_mesh_csr; w = one weight per entry of nb; dist = the bits of the field, one word a vertex; flags: geo_blocks(nv)
// words each.  geo_weights: w, counts[skipped] += the edges without a finite weight, counts[max_edge] = the bits of the
// longest finite one (counts cleared by the host).  geo_seed: dist = +inf, +0.0 at the seeds, is_seed, flag_a raised at
// the blocks of the seeds and their neighbours, flag_b cleared (2 kernels).  geo_round: one round; the blocks flagged in
// cur run and clear their flag, *mark += the flags they raise in next (all 0 before).  geo_pred: pred,
// counts[reached], counts[max_dist].
enum { geo_num_skipped = 0, geo_num_max_edge, geo_num_reached, geo_num_max_dist, geo_num_band_over, geo_num_csr,
       geo_num_words = geo_num_csr + 4 };
size_t     geo_blocks(long long nv);
hipError_t launch_geo_weights(const double* v, const int32_t* off, const int32_t* nb, long long nv, double* w,
                              unsigned long long* counts, hipStream_t s);
hipError_t launch_geo_seed(const int32_t* seeds, long long n_seeds, const int32_t* off, const int32_t* nb, long long nv,
                           unsigned long long* dist, uint8_t* is_seed, unsigned int* flag_a, unsigned int* flag_b,
                           hipStream_t s);
hipError_t launch_geo_round(const int32_t* off, const int32_t* nb, const double* w, long long nv, unsigned long long* dist,
                            unsigned int* cur, unsigned int* next, unsigned long long* mark, hipStream_t s);
hipError_t launch_geo_pred(const int32_t* off, const int32_t* nb, const double* w, const unsigned long long* dist,
                           const uint8_t* is_seed, long long nv, int32_t* pred, unsigned long long* counts, hipStream_t s);
// band skeleton (mm_geodesic_kernels.hip; "Rule S").  geo_sort: keys[0 .. n) ascending, distinct and below ~0, in a buffer
// of geo_sort_size(n) entries (a bitonic network; *launches += its kernels).  skel_bands: band, counts[band_over] set
// where a band index reaches 2^31, link = the hooking union-find over the edges inside a band (2 kernels;
// launch_weld_jump flattens it).  skel_roots: is_root.  skel_keys: keys[ridx[i]] = band << 32 | i at the roots (ridx:
// launch_trim_scan of is_root).  skel_number, behind the sort: node_of_root, rim (from the edge table's counts), vnode,
// nflags (bits 0 and 2), vcnt; ccnt cleared (3 kernels).  skel_faces: area3[f] = a_f / 3, ccnt (1 kernel, none without
// faces).  skel_fill: the corner and vertex lists through the cursors launch_mesh_row_offsets left.  skel_nodes: the
// records, ten 8-byte words a node.  skel_edges: the node pairs through the edge table's keys (cleared here) into out,
// unordered, *n_out their number (2 kernels).
long long  geo_sort_size(long long n);
hipError_t launch_geo_sort(unsigned long long* keys, long long n, int* launches, hipStream_t s);
hipError_t launch_skel_bands(const unsigned long long* dist, long long nv, double h, const int32_t* off, const int32_t* nb,
                             const double* w, int32_t* band, unsigned int* link, unsigned long long* counts, hipStream_t s);
hipError_t launch_skel_roots(const unsigned int* link, const int32_t* band, long long nv, uint8_t* is_root, hipStream_t s);
hipError_t launch_skel_keys(const int32_t* ridx, const int32_t* band, long long nv, long long n_nodes,
                            unsigned long long* keys, hipStream_t s);
hipError_t launch_skel_number(const unsigned long long* keys, long long n_nodes, int32_t* node_of_root,
                              const unsigned long long* ekeys, const unsigned int* ecnt, int log2_cap,
                              const unsigned int* link, const int32_t* band, const uint8_t* is_seed, long long nv,
                              uint8_t* rim, int32_t* vnode, unsigned int* nflags, int32_t* vcnt, int32_t* ccnt, hipStream_t s);
hipError_t launch_skel_faces(const double* v, const int32_t* face, long long nf, const int32_t* vnode, double* area3,
                             int32_t* ccnt, hipStream_t s);
hipError_t launch_skel_fill(const int32_t* face, long long nf, const int32_t* vnode, long long nv, int32_t* ccur,
                            int32_t* clist, int32_t* vcur, int32_t* vlist, hipStream_t s);
hipError_t launch_skel_nodes(long long n_nodes, const int32_t* coff, const int32_t* clist, const int32_t* voff,
                             const int32_t* vlist, const int32_t* face, const double* area3, const double* v,
                             const int32_t* band, const unsigned int* nflags, double* rec, hipStream_t s);
hipError_t launch_skel_edges(const int32_t* off, const int32_t* nb, const double* w, const int32_t* vnode, long long nv,
                             unsigned long long* keys, int log2_cap, unsigned long long* out, unsigned long long* n_out,
                             hipStream_t s);
// rim conditioning (mm_rim_kernels.hip): v = xyz triples, face = int32 triples, index = int32 vertex indices or -1.
// rim_locate: index[k] = the last vertex equal by value to query k (q: 3 r folded bit patterns; index holds -1 before);
// rim_write: v[index[i]] = pts[i]; rim_mark: arr[index[i]] = i (by_position) or 0; rim_layer: ring k of the BFS layers
// (layer: -1 unvisited), *n_new += the vertices set; rim_push: the vertices of layer k >= 1 pushed by k * step;
// rim_gather: out[i] = v[index[i]]; rim_edge_faces: keep[f] = 0 and (f, a, b, c) appended to list (list_cap entries;
// *n_list counts all) for the faces with an edge between ring neighbours (pos: ring position or -1) whose ring edge has
// counts > 0; rim_face_gather: out[fidx[f]] = face f where fidx[f] >= 0 (fidx: launch_trim_scan of keep)
int        rim_locate_chunk_points();
hipError_t launch_rim_locate(const double* v, long long nv, const unsigned long long* q, int r, int32_t* index, hipStream_t s);
hipError_t launch_rim_write(const int32_t* index, const double* pts, int n, double* v, hipStream_t s);
hipError_t launch_rim_mark(const int32_t* index, int n, int by_position, int32_t* arr, hipStream_t s);
hipError_t launch_rim_layer(const int32_t* face, long long nf, int32_t* layer, int32_t k, unsigned int* n_new, hipStream_t s);
hipError_t launch_rim_push(double* v, long long nv, const int32_t* layer, const double o[3], const double n[3], double step,
                           hipStream_t s);
hipError_t launch_rim_gather(const double* v, const int32_t* index, int n, double* out, hipStream_t s);
hipError_t launch_rim_edge_faces(const int32_t* face, long long nf, const int32_t* pos, const int32_t* counts, int n,
                                 uint8_t* keep, int32_t* list, unsigned int list_cap, unsigned int* n_list, hipStream_t s);
hipError_t launch_rim_face_gather(const int32_t* face, long long nf, const int32_t* fidx, int32_t* out, hipStream_t s);
// branch masks (mm_branch_kernels.hip): pts = n xyz triples; cl = m packed centerline points (x, y, z, 1 << branch_id),
// staged through LDS branch_tile_points() at a time; mask[i] = the bits of the centerline points within squared
// distance r2 of point i
hipError_t launch_branch_mask(const double* pts, long long n, const BranchClPoint* cl, int m, double r2,
                              unsigned long long* mask, hipStream_t s);
int        branch_tile_points();
hipError_t launch_exact_all(const BatchDev& b, int max_na, int max_nbp, hipStream_t s);
// bytes between HBM and pinned host memory by a 256-thread kernel (see k_copy_small: a runtime copy behind a
// kernel is a 512-thread blit that starves beside another stream's screen launch); 16-byte aligned pointers
hipError_t launch_copy_small(void* dst, const void* src, size_t bytes, hipStream_t s);
// search sets built on the device: one workgroup per set; writes the four planes of the point pool and, per
// set, the largest squared distance from the centre (rho2) and the largest coordinate magnitude before / after
// centring (scale)
hipError_t launch_build_sets(const SetSrc* src, int n_sets, const double* raw, float* p32x, float* p32y, double* p64x,
                             double* p64y, double* rho2, double* scale, hipStream_t s);
hipError_t launch_shortlist(const BatchDev& b, hipStream_t s);
hipError_t launch_rescore(const BatchDev& b, int max_na, int max_nbp, int total_candidates, hipStream_t s);
hipError_t launch_finalize(const BatchDev& b, int use_flags, hipStream_t s);
// Device-side exchange records of a sharded search (candidate axis split over ranks), indexed by JOB
// (pair_of_job[j] = this level's pair of job j, or -1 when the job takes no part in the level):
//   export_cost  cost[j] = exact first-minimum cost inside this rank's slice, +inf if it holds no candidate
//                -> all-reduce(MIN) over the ranks gives the global best cost
//   export_keys  given the reduced costs g: keys[j] = first-minimum index if this rank attains g[j], else
//                INT64_MAX; keys[n+j], keys[2n+j] = (angle bits, ~angle bits) of the rank's winner if its
//                minimum lies within the pair's tie tolerance of g[j] and all its near-ties are one angle
//                value, (INT64_MIN, INT64_MIN) if they are not, (INT64_MAX, INT64_MAX) if it is not near
//                -> ONE all-reduce(MIN) of the 3n keys gives the first index of minimal cost over the whole
//                axis (process_utils.rs:72) and min / ~max of the near ranks' angle bits (equal <=> decided)
hipError_t launch_export_cost(const BatchDev& b, const int32_t* pair_of_job, int n_jobs, double* cost, hipStream_t s);
hipError_t launch_export_keys(const BatchDev& b, const int32_t* pair_of_job, int n_jobs, const double* gcost,
                              long long* keys, hipStream_t s);

// closed smoothing B-spline contours (mm_bspline_kernels.hip): one job per contour (first point, count), one wave
// each, the work arrays of a contour in lds_bytes = 8 * bspline_work_doubles(longest m, k) of dynamic LDS.
// out_xyz is indexed like xyz; status / fp / nknots per job.
size_t     bspline_work_doubles(int m, int k);
hipError_t launch_bspline_fit(const BsplJob* jobs, int n_jobs, const double* xyz, int k, double s, size_t lds_bytes,
                              double* out_xyz, int32_t* status, double* fp, int32_t* nknots, hipStream_t st);

}  // namespace mm
