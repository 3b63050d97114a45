// mm_shape.cpp -- lumen morphometry (include/mm_build.h): the per-contour measures of src/types/native/contour.rs on
// the device (mm_shape_kernels.hip, every contour of a batch in one launch) and the summary rule of
// src/types/binding/py_geometry.rs:190-260 on the host.  The 2-D closest-opposite angles are taken here with
// std::atan2 (the device's atan2 is not the C library's) on the worker pool, one contour per slot; everything after
// them is exact on the device.  Host f64 is built with -ffp-contract=off, in the reference's operation order.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mm_build.h"
#include "mm_stage.h"
#include "mm_pool.h"

namespace mm {
namespace {

// find_closest_opposite (contour.rs:247-273): the centre is the stored centroid, else the sequential mean of the
// points; theta = atan2(y - cy, x - cx), + 2 pi below 0
void opposite_angles(const double* p, int64_t n, const double* centre, double* theta)
{
    double cx, cy;
    if (centre) {
        cx = centre[0];
        cy = centre[1];
    } else {
        double sx = 0.0, sy = 0.0;
        for (int64_t k = 0; k < n; ++k) { sx += p[3 * k]; sy += p[3 * k + 1]; }
        cx = sx / (double)n;
        cy = sy / (double)n;
    }
    for (int64_t k = 0; k < n; ++k) {
        double t = std::atan2(p[3 * k + 1] - cy, p[3 * k] - cx);
        if (t < 0.0) t += 2.0 * M_PI;
        theta[k] = t;
    }
}

int contour_measures(Engine* e, int64_t nc, const int64_t* off, const double* xyz, const uint8_t* has_centroid,
                     const double* centroid, bool want2d, double* out_val, int64_t* out_idx)
{
    const int64_t NP = off[nc];
    std::vector<ShapeJob> jobs((size_t)nc);
    double evals = 0.0;
    for (int64_t c = 0; c < nc; ++c) {
        const int64_t n = off[c + 1] - off[c];
        jobs[(size_t)c] = ShapeJob{off[c], (int32_t)n, 0};
        evals += 0.5 * (double)n * (double)(n > 0 ? n - 1 : 0) + (want2d ? (double)n * (double)n : 0.0);
    }
    StagedPass sp;
    const size_t o_xyz = sp.in.take((size_t)NP * 24), o_t = sp.in.take(want2d ? (size_t)NP * 8 : 0);
    const size_t o_jobs = sp.in.take((size_t)nc * sizeof(ShapeJob));
    const size_t o_val = sp.out.take((size_t)nc * 40), o_idx = sp.out.take((size_t)nc * 48);
    int rc = sp.reserve(e);
    if (rc) return rc;
    if (NP) std::memcpy(sp.host<double>(o_xyz), xyz, (size_t)NP * 24);
    if (want2d) {
        double* th = sp.host<double>(o_t);
        WorkerPool::instance().parallel_for((int)nc, [&](int c) {
            const int64_t n = off[c + 1] - off[c];
            if (n < 3) return;                                                     // the 2-D pass needs n > 2
            const bool own = has_centroid && has_centroid[c];
            opposite_angles(xyz + 3 * off[c], n, own ? centroid + 3 * (size_t)c : nullptr, th + off[c]);
        });
    }
    std::memcpy(sp.host<ShapeJob>(o_jobs), jobs.data(), jobs.size() * sizeof(ShapeJob));
    rc = sp.run(evals, "contour measures launch", [&] {
        return launch_contour_measures(sp.dev_in<ShapeJob>(o_jobs), (int)nc, sp.dev_in<double>(o_xyz),
                                       want2d ? sp.dev_in<double>(o_t) : nullptr, want2d ? 1 : 0,
                                       sp.dev_out<double>(o_val), sp.dev_out<int64_t>(o_idx), e->stream);
    });
    if (rc) return rc;
    std::memcpy(out_val, sp.host<double>(o_val), (size_t)nc * 40);
    std::memcpy(out_idx, sp.host<int64_t>(o_idx), (size_t)nc * 48);
    return MM_OK;
}

}  // namespace
}  // namespace mm

using namespace mm;

extern "C" {

int mm_contour_measures(mm_engine* h, int64_t n_contours, const int64_t* off, const double* xyz,
                        const uint8_t* has_centroid, const double* centroid_xyz, uint32_t flags, double* out_val,
                        int64_t* out_idx)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (n_contours < 0 || (flags & ~(uint32_t)MM_MEASURE_CLOSEST_2D) || (has_centroid && !centroid_xyz) ||
        (n_contours > 0 && (!off || !out_val || !out_idx)))
        return set_error(MM_ERR_INVALID, "mm_contour_measures: bad arguments");
    if (n_contours == 0) return MM_OK;
    if (n_contours > INT32_MAX / 2) return set_error(MM_ERR_TOO_LARGE, "mm_contour_measures: too many contours");
    if (off[0] != 0) return set_error(MM_ERR_INVALID, "mm_contour_measures: offsets must start at 0 and not decrease");
    for (int64_t c = 0; c < n_contours; ++c) {
        if (off[c + 1] < off[c])
            return set_error(MM_ERR_INVALID, "mm_contour_measures: offsets must start at 0 and not decrease");
        if (off[c + 1] - off[c] > INT32_MAX / 4)
            return set_error(MM_ERR_TOO_LARGE, "mm_contour_measures: a contour has too many points");
    }
    if (off[n_contours] > 0 && !xyz) return set_error(MM_ERR_INVALID, "mm_contour_measures: bad arguments");
    return contour_measures(e, n_contours, off, xyz, has_centroid, centroid_xyz,
                            (flags & MM_MEASURE_CLOSEST_2D) != 0, out_val, out_idx);
}

// PyGeometry::get_summary (py_geometry.rs:190-260)
int mm_summary_from_measures(int64_t n_frames, const double* area, const double* ratio, const int64_t* n_points,
                             const double* centroids_xyz, double* out)
{
    if (!out || n_frames < 0 || (n_frames > 0 && (!area || !ratio || !n_points || !centroids_xyz)))
        return set_error(MM_ERR_INVALID, "mm_summary_from_measures: bad arguments");
    out[0] = out[1] = out[2] = 0.0;
    if (n_frames == 0) return MM_OK;                                                      // :193-195
    double biggest = NAN, mla = INFINITY;                                                 // :200-201 f64::max / f64::min
    for (int64_t k = 0; k < n_frames; ++k) {
        const double a = area[k];
        if (std::isnan(biggest) || a > biggest) biggest = std::isnan(a) ? biggest : a;
        if (!std::isnan(a) && a < mla) mla = a;
    }
    const double max_stenosis = biggest > 0.0 ? 1.0 - (mla / biggest) : 0.0;            // :202-206
    bool all_elliptic = true;                                                             // :209-212, short-circuit
    for (int64_t k = 0; k < n_frames && all_elliptic; ++k) {
        if (n_points[k] == 0)
            return set_error(MM_ERR_INVALID, "get_summary: frame " + std::to_string(k) +
                             " has an empty lumen contour (its farthest points are undefined)");
        if (n_points[k] < 3)
            return set_error(MM_ERR_INVALID, "get_summary: frame " + std::to_string(k) +
                             " has a lumen contour of fewer than 3 points (its elliptic ratio is undefined)");
        all_elliptic = ratio[k] < 1.3;
    }
    const double threshold = all_elliptic ? 0.70 * biggest : 0.50 * biggest;            // :214-218
    double longest = 0.0;                                                                 // :223-250
    int64_t i = 0;
    while (i < n_frames) {
        if (area[i] < threshold) {
            const int64_t start = i;
            int64_t end = i;
            while (end + 1 < n_frames && area[end + 1] < threshold) ++end;
            double run = 0.0;
            for (int64_t k = start; k < end; ++k) {
                const double* a = centroids_xyz + 3 * k;
                const double* b = a + 3;
                const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
                run += std::sqrt(dx * dx + dy * dy + dz * dz);
            }
            if (run > longest) longest = run;
            i = end + 1;
        } else {
            ++i;
        }
    }
    out[0] = mla;
    out[1] = max_stenosis;
    out[2] = longest;
    return MM_OK;
}

}  // extern "C"
