// mm_bspline_kernels.hip -- closed smoothing B-spline contours (mm_bspline_fit_closed_batch, include/mm_ccta.h), gfx950.
//
// One wave per contour, every contour of the batch in one launch.  The contour's whole problem -- its points, the
// parameter, the knots, the band matrix with its border columns, the copy the smoothing iteration rotates the
// discontinuity rows into, the right-hand sides and the basis values at the data sites -- stays in the block's LDS
// (bspl::work_doubles(m, k) doubles, sized by the longest contour of the batch; MM_BSPLINE_MAX_POINTS keeps that inside
// the 160 KB a gfx950 block may take).  Lane 0 runs the whole fit (mm_bspline_fit.h: basis values, Givens elimination,
// knot insertion, the search for p), in exactly the checker's operation order; only the m evaluation points are spread
// over the 64 lanes.  The batch is what runs in parallel, not the contour (DESIGN 4.17 says what that costs).  f64
// throughout, never fused (-ffp-contract=off).
#include <hip/hip_runtime.h>

#include "mm_bspline_fit.h"
#include "mm_device.h"

namespace mm {

__global__ void __launch_bounds__(64)
k_bspline_fit(const BsplJob* __restrict__ jobs, int n_jobs, const double* __restrict__ xyz, int k, double s,
              double* __restrict__ out_xyz, int32_t* __restrict__ status, double* __restrict__ fp,
              int32_t* __restrict__ nknots)
{
    extern __shared__ double lds[];
    __shared__ int sh_status, sh_n, sh_bad;
    const int j = (int)blockIdx.x;
    if (j >= n_jobs) return;
    const BsplJob job = jobs[j];
    bspl::Work w;
    bspl::carve(lds, job.m, k, w);
    if (threadIdx.x == 0) {
        int n = 0;
        double f = 0.0;
        sh_status = bspl::fit(xyz + 3 * (size_t)job.p_off, job.m, k, s, w, n, f);
        sh_n = n;
        sh_bad = 0;
        fp[j] = f;
        if (!isfinite(f)) sh_bad = 1;
    }
    __syncthreads();
    const int st = sh_status, n = sh_n;
    const bool curve = st == bspl::kFitted || st == bspl::kInterpolated || st == bspl::kCollapsed || st == bspl::kIterationLimit;
    if (curve) {
        for (int i = (int)threadIdx.x; i < job.m; i += 64) {
            double o[3];
            const bool ok = bspl::evaluate(w.t, w.c, n, k, job.m, i, o);
            if (!ok || !isfinite(o[0]) || !isfinite(o[1]) || !isfinite(o[2])) atomicOr(&sh_bad, 1);
            double* dst = out_xyz + 3 * ((size_t)job.p_off + (size_t)i);
            dst[0] = o[0]; dst[1] = o[1]; dst[2] = o[2];
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        status[j] = (curve && sh_bad) ? (int32_t)bspl::kUnchangedNonFinite : (int32_t)st;
        nknots[j] = curve && !sh_bad ? n : 0;
    }
}

size_t bspline_work_doubles(int m, int k) { return bspl::work_doubles(m, k); }

hipError_t launch_bspline_fit(const BsplJob* jobs, int n_jobs, const double* xyz, int k, double s, size_t lds_bytes,
                              double* out_xyz, int32_t* status, double* fp, int32_t* nknots, hipStream_t st)
{
    if (n_jobs <= 0) return hipSuccess;
    if (lds_bytes > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)k_bspline_fit, hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)lds_bytes);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_bspline_fit, dim3((unsigned)n_jobs), dim3(64), lds_bytes, st, jobs, n_jobs, xyz, k,
                       s, out_xyz, status, fp, nknots);
    return hipGetLastError();
}

}  // namespace mm
