// mm_slice_kernels.hip -- Voronoi slicing of a vessel surface along its centerline, exact f64, for gfx950.
//
// walk_centerline_slices (src/ccta/discretizing/projecting.rs:13-101) assigns every mesh point to its nearest slice
// anchor and projects it onto that anchor's plane.  Per point p of a job and that job's anchors a_0 .. a_{M-1}:
//   d_j = (px - ax)^2 + (py - ay)^2 + (pz - az)^2        sq_dist3 (:121): three products, (dx^2 + dy^2) + dz^2
//   best = the fold of min_by with partial_cmp().unwrap_or(Equal) (:70-89): start at anchor 0, anchor j replaces
//          the current best iff best > d_j.  Ties keep the lowest index; a NaN d_0 pins the point to anchor 0; a NaN
//          d_j (j > 0) is never chosen.
//   s = ((px - cx) nx + (py - cy) ny) + (pz - cz) nz,  q = p - n s      project_to_plane (:106-118), nalgebra's dot
// No contraction (the file is built with -ffp-contract=off), so every value is the reference's bit for bit.
//
// Mapping: one work item = one job x 256 consecutive points (one per lane).  Each lane folds its own point over the
// job's whole anchor range in anchor order (nearest_fold, mm_point_device.h: anchors staged through LDS in tiles), so the
// tie and NaN rules hold without a cross-lane merge and no atomics are needed.  Many jobs (aorta, main vessels, side
// branches) share one launch; work items are job-major and dealt to the XCDs in contiguous eighths.
#include <hip/hip_runtime.h>

#include "mm_device.h"
#include "mm_point_device.h"
#include "mm_xcd.h"

namespace mm {

// pts: xyz triples; anc: 6 doubles per anchor (x, y, z, nx, ny, nz); idx / proj: per point, at the point's position
__global__ void __launch_bounds__(256)
k_slice_nearest(const SliceJob* __restrict__ jobs, const PointWork* __restrict__ work, int n_work,
                const double* __restrict__ pts, const double* __restrict__ anc, int32_t* __restrict__ idx,
                double* __restrict__ proj)
{
    const int tid = threadIdx.x;
    for (int wi = (int)gridDim.x == n_work ? xcd_work_index(blockIdx.x, n_work) : (int)blockIdx.x; wi < n_work;
         wi += gridDim.x) {
        const PointWork w = work[wi];
        const SliceJob jb = jobs[w.job];
        const int i = w.p0 + tid;
        const size_t pi = (size_t)jb.p_off + (size_t)(i < jb.np ? i : jb.np - 1);   // lanes past the end recompute the last point
        const double px = pts[3 * pi], py = pts[3 * pi + 1], pz = pts[3 * pi + 2];
        const double* a0 = anc + 6 * (size_t)jb.a_off;
        const double dx = px - a0[0], dy = py - a0[1], dz = pz - a0[2];
        // the fold's start: d_0, which anchor 0 itself never beats
        const int bi = nearest_fold<6>(a0, jb.na, px, py, pz, dx * dx + dy * dy + dz * dz);
        if (i < jb.np) {
            const double* a = a0 + 6 * (size_t)bi;
            const double cx = a[0], cy = a[1], cz = a[2], nx = a[3], ny = a[4], nz = a[5];
            const double s = ((px - cx) * nx + (py - cy) * ny) + (pz - cz) * nz;
            idx[pi] = bi;
            proj[3 * pi] = px - nx * s;
            proj[3 * pi + 1] = py - ny * s;
            proj[3 * pi + 2] = pz - nz * s;
        }
    }
}

int slice_block_points() { return kNearestLanes; }

hipError_t launch_slice_nearest(const SliceJob* jobs, const PointWork* work, int n_work, const double* pts,
                                const double* anc, int32_t* idx, double* proj, hipStream_t s)
{
    if (n_work <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_slice_nearest, dim3((unsigned)n_work), dim3(256), 0, s, jobs, work, n_work, pts, anc, idx, proj);
    return hipGetLastError();
}

}  // namespace mm
