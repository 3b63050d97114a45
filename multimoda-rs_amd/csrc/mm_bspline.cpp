// mm_bspline.cpp -- closed smoothing B-spline contours (include/mm_ccta.h, "B-spline contours").  Reference:
// multimodars/ccta/discretization_map.py:16-101 (_fit_bspline_contour, _replace_contours_with_bsplines), i.e. scipy's
// splprep(per=True) + splev; the fit itself is mm_bspline_fit.h, run by mm_bspline_kernels.hip for every contour of the
// batch in one launch.  The host screens what needs no arithmetic (too short, non-finite), stages the rest once, and
// takes the centroids in numpy's pairwise order.
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/mm_ccta.h"
#include "mm_device.h"
#include "mm_stage.h"

namespace mm {
namespace {

// numpy's pairwise sum of n doubles `stride` apart: fewer than 8 one after the other; up to 128 in eight accumulators
// combined ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), the rest one after the other; longer arrays split at n/2 rounded down
// to a multiple of 8
double pairwise_sum(const double* a, int64_t n, int64_t stride)
{
    if (n < 8) {
        double r = -0.0;
        for (int64_t i = 0; i < n; ++i) r = r + a[i * stride];
        return r;
    }
    if (n <= 128) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j * stride];
        int64_t i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] = r[j] + a[(i + j) * stride];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res = res + a[i * stride];
        return res;
    }
    int64_t n2 = n / 2;
    n2 -= n2 % 8;
    return pairwise_sum(a, n2, stride) + pairwise_sum(a + n2 * stride, n - n2, stride);
}

}  // namespace
}  // namespace mm

using namespace mm;

extern "C" {

int mm_bspline_fit_closed_batch(mm_engine* h, int64_t n_contours, const double* xyz, const int64_t* offsets,
                                double smoothing, int degree, double* out_xyz, double* out_centroid,
                                int32_t* out_status, double* out_fp, int32_t* out_nknots)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (n_contours < 0 || n_contours > kMaxIndex || (n_contours > 0 && (!offsets || !out_centroid || !out_status || !out_fp || !out_nknots)))
        return set_error(MM_ERR_INVALID, "mm_bspline_fit_closed_batch: bad arguments");
    if (degree < 1 || degree > 5)
        return set_error(MM_ERR_INVALID, "mm_bspline_fit_closed_batch: degree must be in 1..5");
    if (!(smoothing >= 0.0) || !std::isfinite(smoothing))
        return set_error(MM_ERR_INVALID, "mm_bspline_fit_closed_batch: smoothing must be finite and >= 0");
    if (n_contours == 0) return MM_OK;
    const int nc = (int)n_contours;
    if (!offsets_ok(offsets, nc))
        return set_error(MM_ERR_INVALID, "mm_bspline_fit_closed_batch: offsets must start at 0 and not decrease");
    const int64_t NP = offsets[nc];
    if (NP > kMaxIndex / 4) return set_error(MM_ERR_TOO_LARGE, "mm_bspline_fit_closed_batch: too many points for one pass");
    if (NP > 0 && (!xyz || !out_xyz)) return set_error(MM_ERR_INVALID, "mm_bspline_fit_closed_batch: bad arguments");
    int m_max = 0;
    for (int j = 0; j < nc; ++j) {
        const int64_t m = offsets[j + 1] - offsets[j];
        if (m > MM_BSPLINE_MAX_POINTS)
            return set_error(MM_ERR_INVALID, "mm_bspline_fit_closed_batch: a contour has more than MM_BSPLINE_MAX_POINTS points");
        if ((int)m > m_max) m_max = (int)m;
    }
    const size_t wd = bspline_work_doubles(m_max, degree);
    int lds_cap = 0;
    MM_TRY_HIP(hipDeviceGetAttribute(&lds_cap, hipDeviceAttributeMaxSharedMemoryPerBlock, e->device));
    if (wd * 8 + 64 > (size_t)lds_cap)
        return set_error(MM_ERR_TOO_LARGE, "mm_bspline_fit_closed_batch: the longest contour's system does not fit the "
                                           "device's LDS per block");
    // from here on the outputs are written.  Unchanged contours: the input, fp 0, no knots.
    std::vector<BsplJob> jobs;
    std::vector<int> job_of;                       // contour of each job
    for (int j = 0; j < nc; ++j) {
        const int64_t lo = offsets[j], m = offsets[j + 1] - lo;
        out_fp[j] = 0.0;
        out_nknots[j] = 0;
        if (m) std::memcpy(out_xyz + 3 * lo, xyz + 3 * lo, (size_t)m * 24);
        if (m < degree + 1) { out_status[j] = MM_BSPLINE_UNCHANGED_SHORT; continue; }
        bool finite = true;
        for (int64_t i = 3 * lo; i < 3 * (lo + m); ++i) finite = finite && std::isfinite(xyz[i]);
        if (!finite) { out_status[j] = MM_BSPLINE_UNCHANGED_NONFINITE; continue; }
        out_status[j] = MM_BSPLINE_FITTED;
        jobs.push_back(BsplJob{(int32_t)lo, (int32_t)m});
        job_of.push_back(j);
    }
    if (!jobs.empty()) {
        const int nj = (int)jobs.size();
        StagedPass sp;
        const size_t o_xyz = sp.in.take((size_t)NP * 24), o_jobs = sp.in.take((size_t)nj * sizeof(BsplJob));
        const size_t o_out = sp.out.take((size_t)NP * 24), o_fp = sp.out.take((size_t)nj * 8);
        const size_t o_st = sp.out.take((size_t)nj * 4), o_nk = sp.out.take((size_t)nj * 4);
        if ((rc = sp.reserve(e))) return rc;
        std::memcpy(sp.host<double>(o_xyz), xyz, (size_t)NP * 24);
        std::memcpy(sp.host<BsplJob>(o_jobs), jobs.data(), (size_t)nj * sizeof(BsplJob));
        rc = sp.run((double)NP, "B-spline fit launch", [&] {
            return launch_bspline_fit(sp.dev_in<BsplJob>(o_jobs), nj, sp.dev_in<double>(o_xyz), degree, smoothing, wd * 8,
                                      sp.dev_out<double>(o_out), sp.dev_out<int32_t>(o_st), sp.dev_out<double>(o_fp),
                                      sp.dev_out<int32_t>(o_nk), e->stream);
        });
        if (rc) return rc;
        for (int q = 0; q < nj; ++q) {
            const int j = job_of[(size_t)q];
            const int32_t st = sp.host<int32_t>(o_st)[q];
            out_status[j] = st;
            if (st == MM_BSPLINE_UNCHANGED_SHORT || st == MM_BSPLINE_UNCHANGED_ZERO_CHORD || st == MM_BSPLINE_UNCHANGED_NONFINITE)
                continue;
            if (st < 0 || st > MM_BSPLINE_ITERATION_LIMIT) return set_error(MM_ERR_HIP, "mm_bspline_fit_closed_batch: bad status from the device");
            out_fp[j] = sp.host<double>(o_fp)[q];
            out_nknots[j] = sp.host<int32_t>(o_nk)[q];
            const size_t lo = (size_t)jobs[(size_t)q].p_off;
            std::memcpy(out_xyz + 3 * lo, sp.host<double>(o_out) + 3 * lo, (size_t)jobs[(size_t)q].m * 24);
        }
    }
    for (int j = 0; j < nc; ++j) {                 // np.mean of each coordinate of the contour as returned
        const int64_t lo = offsets[j], m = offsets[j + 1] - lo;
        for (int dd = 0; dd < 3; ++dd)
            out_centroid[3 * j + dd] = m ? (0.0 + pairwise_sum(out_xyz + 3 * lo + dd, m, 3)) / (double)m : std::nan("");
    }
    return MM_OK;
}

int mm_bspline_max_points(void) { return MM_BSPLINE_MAX_POINTS; }

}  // extern "C"
