// mm_point_records.h -- the device records of the CCTA point kernels (mm_nn, mm_tri, mm_ray, mm_slice, mm_morph,
// mm_shape, mm_branch, mm_bspline _kernels.hip), declared once for those kernels and for the host files that fill them
// (mm_ccta, mm_surface, mm_discretize, mm_shape, mm_branch, mm_bspline .cpp); mm_device.h's launchers take them by type.
// Plain C++; internal.
#pragma once

#include <cstdint>

namespace mm {

// mm_nn_kernels.hip.  q_off / p_off: into the point pool; out_off: into the output; qperm_off: into the permutation pool (the
// staged position j of the query set holds original point qperm[qperm_off + j]; -1 = staged in original order)
struct NnPair { int32_t q_off, nq, p_off, np, out_off, qperm_off; };
// queries [q0, q0 + nn_queries_per_block()) x points [c0, c0 + n_chunks nn_chunk_points()); lb2: the bound of
// mm_prune.h (box_lb2) between the two; pass B of k_nn3_min reads it, pass A stores 0
struct NnWork { int32_t pair, q0, c0, n_chunks; double lb2; };
// A derived set: pool[dst_off + j] = aux point aux_off + j moved by adj along its unit vector where its flag is set
struct NnMorph { int32_t dst_off, n, aux_off, pad; double adj; };
// mm_tri_kernels.hip: queries [q0, q0 + tri_queries_per_block()) x faces [c0, c0 + tri_chunk_faces()), both in staged
// order; lb2: the bound of mm_prune.h (box_lb2) between the two (pass B and the who pass of k_tri_min read it)
struct TriWork { int32_t q0, c0; double lb2; };
// mm_ray_kernels.hip: hits of one ray in one chunk of faces, closest (t, face)
struct RayPartial { int32_t count, face; double t; };
// mm_slice_kernels.hip, mm_morph_kernels.hip: points [p0, p0 + *_block_points()) of job `job`
struct PointWork { int32_t job, p0; };
struct SliceJob { int32_t p_off, np, a_off, na; };               // points [p_off, p_off + np), anchors [a_off, a_off + na)
struct MorphJob { int32_t p_off, np, c_off, nc; double adj; };   // points [p_off, p_off + np), centerline [c_off, c_off + nc)
// mm_shape_kernels.hip: points [off, off + n) of one contour
struct ShapeJob { int64_t off; int32_t n; int32_t pad; };
// mm_branch_kernels.hip: one packed centerline point, bit = 1 << branch_id; two 16-byte LDS reads
struct alignas(32) BranchClPoint { double x, y, z; unsigned long long bit; };
// mm_bspline_kernels.hip: first point and point count of one contour
struct BsplJob { int32_t p_off, m; };

static_assert(sizeof(NnPair) == 24 && alignof(NnPair) == 4, "NnPair layout");
static_assert(sizeof(NnWork) == 24 && alignof(NnWork) == 8, "NnWork layout");
static_assert(sizeof(TriWork) == 16 && alignof(TriWork) == 8, "TriWork layout");
static_assert(sizeof(NnMorph) == 24 && alignof(NnMorph) == 8, "NnMorph layout");
static_assert(sizeof(RayPartial) == 16 && alignof(RayPartial) == 8, "RayPartial layout");
static_assert(sizeof(PointWork) == 8 && alignof(PointWork) == 4, "PointWork layout");
static_assert(sizeof(SliceJob) == 16 && alignof(SliceJob) == 4, "SliceJob layout");
static_assert(sizeof(MorphJob) == 24 && alignof(MorphJob) == 8, "MorphJob layout");
static_assert(sizeof(ShapeJob) == 16 && alignof(ShapeJob) == 8, "ShapeJob layout");
static_assert(sizeof(BranchClPoint) == 32 && alignof(BranchClPoint) == 32, "BranchClPoint layout");
static_assert(sizeof(BsplJob) == 8 && alignof(BsplJob) == 4, "BsplJob layout");

}  // namespace mm
