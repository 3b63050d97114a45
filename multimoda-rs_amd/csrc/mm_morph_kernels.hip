// mm_morph_kernels.hip -- radial morphing of mesh vertices about their nearest centerline point, exact f64, for gfx950.
//
// centerline_based_diameter_morphing (src/ccta/adjust_mesh/scale_coronary.rs:218-260).  Per point p of a job, that
// job's centerline points c_0 .. c_{M-1} (M >= 1) and its adjustment a:
//   d_j = (px - cx)^2 + (py - cy)^2 + (pz - cz)^2        calculate_squared_distance: three products, (dx^2 + dy^2) + dz^2
//   k   = find_closest_centerline_point_optimized (:245-260): best = DBL_MAX, index 0; c_j replaces the best iff
//         d_j < best.  Ties keep the lowest index; a NaN d_j is never chosen; if no d_j is below DBL_MAX the point
//         keeps index 0.  (Not k_slice_nearest's fold, which starts from d_0.)
//   v = p - c_k,  n = sqrt((vx^2 + vy^2) + vz^2)          try_normalize(0.0) (:236-239)
//   q = p + (v / n) * a  if n > 0, else p                 three correctly rounded divisions; a NaN n keeps p (the rule
//                                                         of the host mm_diameter_morphing and of the oracle)
// No contraction (the file is built with -ffp-contract=off), so every value is the reference's bit for bit; sqrt and
// the divisions are hipcc's correctly rounded expansions (v_rsq_f64 + refinement, v_div_scale/fmas/fixup).
//
// Mapping: one work item = one job x 256 consecutive points (one per lane).  Each lane folds its own point over the
// job's whole centerline range in order (nearest_fold, mm_point_device.h: centerline points staged through LDS in
// tiles), so the tie and NaN rules hold without a cross-lane merge and no atomics are needed.  Many jobs share one
// launch; work items are job-major and dealt to the XCDs in contiguous eighths.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "mm_device.h"
#include "mm_point_device.h"
#include "mm_xcd.h"

namespace mm {

// pts, cl, out: xyz triples; nearest / out at the point's position
__global__ void __launch_bounds__(256)
k_cl_morph(const MorphJob* __restrict__ jobs, const PointWork* __restrict__ work, int n_work,
           const double* __restrict__ pts, const double* __restrict__ cl, int32_t* __restrict__ nearest,
           double* __restrict__ out)
{
    const int tid = threadIdx.x;
    for (int wi = (int)gridDim.x == n_work ? xcd_work_index(blockIdx.x, n_work) : (int)blockIdx.x; wi < n_work;
         wi += gridDim.x) {
        const PointWork w = work[wi];
        const MorphJob jb = jobs[w.job];
        const int i = w.p0 + tid;
        const size_t pi = (size_t)jb.p_off + (size_t)(i < jb.np ? i : jb.np - 1);   // lanes past the end recompute the last point
        const double px = pts[3 * pi], py = pts[3 * pi + 1], pz = pts[3 * pi + 2];
        const double* c0 = cl + 3 * (size_t)jb.c_off;
        const int bi = nearest_fold<3>(c0, jb.nc, px, py, pz, DBL_MAX);       // the start: no d_j below DBL_MAX keeps index 0
        if (i < jb.np) {
            const double* c = c0 + 3 * (size_t)bi;
            const double vx = px - c[0], vy = py - c[1], vz = pz - c[2];
            const double nn = sqrt(vx * vx + vy * vy + vz * vz);
            double qx = px, qy = py, qz = pz;
            if (nn > 0.0) {
                qx = px + (vx / nn) * jb.adj;
                qy = py + (vy / nn) * jb.adj;
                qz = pz + (vz / nn) * jb.adj;
            }
            nearest[pi] = bi;
            out[3 * pi] = qx;
            out[3 * pi + 1] = qy;
            out[3 * pi + 2] = qz;
        }
    }
}

int morph_block_points() { return kNearestLanes; }

hipError_t launch_cl_morph(const MorphJob* jobs, const PointWork* work, int n_work, const double* pts, const double* cl,
                           int32_t* nearest, double* out, hipStream_t s)
{
    if (n_work <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_cl_morph, dim3((unsigned)n_work), dim3(256), 0, s, jobs, work, n_work, pts, cl, nearest, out);
    return hipGetLastError();
}

}  // namespace mm
