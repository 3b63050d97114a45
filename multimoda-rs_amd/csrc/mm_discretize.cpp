// mm_discretize.cpp -- CCTA vessel discretisation (include/mm_ccta.h): uniform cross-sections of a labelled vessel
// surface along its centerline.  Reference: src/ccta/discretizing/{projecting,resampling}.rs (lines cited per
// function).  The slice anchors and the spline resampling are host f64 in the reference's operation order (built with
// -ffp-contract=off); the nearest-anchor assignment and the plane projection run on the device in exact f64
// (mm_slice_kernels.hip), every job of a batch in one launch.  Contours are resampled on the worker pool; each
// writes its own slot, so the result does not depend on the number of workers.
//
// Small-vector arithmetic follows nalgebra (see mm_centerline.cpp): dot = (x0 y0 + x1 y1) + x2 y2, norm = sqrt(dot),
// normalize = v / norm, cross = (ay bz - az by, az bx - ax bz, ax by - ay bx).
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/mm_ccta.h"
#include "mm_stage.h"
#include "mm_pool.h"

namespace mm {
namespace {

struct V3 { double x, y, z; };
inline V3 sub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 add(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline V3 mul(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
inline V3 dvs(V3 a, double s) { return {a.x / s, a.y / s, a.z / s}; }
inline double dot(V3 a, V3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
inline double norm(V3 a) { return std::sqrt(dot(a, a)); }
inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline V3 at(const double* p, int64_t i) { return {p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }

// ---- anchors (projecting.rs:13-60, 123-200) -------------------------------------------------------------------------

// The anchors of branch `branch` walked every `step`: 6 doubles each (position, unit tangent), slice index = position in
// the list.  An absent branch or a NaN total length gives none; a step <= 0 or non-finite (the reference's loop never
// ends) or more than MM_SLICE_MAX_ANCHORS anchors is MM_ERR_INVALID.
int slice_anchors(const mm_clpoint* cl, int64_t ncl, uint32_t branch, double step, std::vector<double>* anc, int64_t& count)
{
    count = 0;
    if (!(step > 0.0) || !std::isfinite(step)) return set_error(MM_ERR_INVALID, "discretize: step_size must be finite and > 0");
    std::vector<const mm_clpoint*> bp;                                          // :19-23 the branch's points in order
    for (int64_t i = 0; i < ncl; ++i)
        if (cl[i].branch_id == branch) bp.push_back(cl + i);
    if (bp.empty()) return MM_OK;
    std::vector<double> cum(1, 0.0);                                             // branch_cum_arc (:123-130)
    for (size_t i = 1; i < bp.size(); ++i) {
        const double dx = bp[i - 1]->x - bp[i]->x, dy = bp[i - 1]->y - bp[i]->y, dz = bp[i - 1]->z - bp[i]->z;
        cum.push_back(cum.back() + std::sqrt(dx * dx + dy * dy + dz * dz));      // distance_to (native.rs:27-32)
    }
    const double total = cum.back();
    if (std::isnan(total)) return MM_OK;                                         // `s <= NaN` never holds: no position
    if (!(total / step <= (double)MM_SLICE_MAX_ANCHORS))
        return set_error(MM_ERR_INVALID, "discretize: total length / step_size exceeds MM_SLICE_MAX_ANCHORS");
    std::vector<double> pos;                                                     // build_sample_positions (:132-146)
    for (double s = 0.0; s <= total + 1e-9; s += step) {
        if ((int64_t)pos.size() >= MM_SLICE_MAX_ANCHORS)
            return set_error(MM_ERR_INVALID, "discretize: more than MM_SLICE_MAX_ANCHORS anchors");
        pos.push_back(s);
    }
    if (!pos.empty() && pos.back() > total + 1e-6) pos.back() = total;
    count = (int64_t)pos.size();
    if (!anc) return MM_OK;
    anc->resize(pos.size() * 6);
    const size_t n = bp.size();
    for (size_t k = 0; k < pos.size(); ++k) {                                    // interpolate_branch_at_s (:148-200)
        const double target = pos[k];
        // binary_search_by over a sorted cum: Ok(i) -> i, Err(0) -> 0, Err(pos) -> pos - 1 == upper_bound - 1
        const size_t ub = (size_t)(std::upper_bound(cum.begin(), cum.end(), target) - cum.begin());
        const size_t seg = ub == 0 ? 0 : ub - 1;
        double* o = anc->data() + 6 * k;
        if (seg >= n - 1) {                                                      // :160-172 the last point as it is
            const mm_clpoint& l = *bp[n - 1];
            o[0] = l.x; o[1] = l.y; o[2] = l.z; o[3] = l.tx; o[4] = l.ty; o[5] = l.tz;
            continue;
        }
        const mm_clpoint &p0 = *bp[seg], &p1 = *bp[seg + 1];
        const double s0 = cum[seg], s1 = cum[seg + 1];
        const double t = std::fabs(s1 - s0) < 1e-12 ? 0.0 : (target - s0) / (s1 - s0);
        V3 tg = add(mul(V3{p0.tx, p0.ty, p0.tz}, 1.0 - t), mul(V3{p1.tx, p1.ty, p1.tz}, t));
        const double nn = norm(tg);
        if (nn > 1e-12) tg = dvs(tg, nn);
        o[0] = p0.x + t * (p1.x - p0.x); o[1] = p0.y + t * (p1.y - p0.y); o[2] = p0.z + t * (p1.z - p0.z);
        o[3] = tg.x; o[4] = tg.y; o[5] = tg.z;
    }
    return MM_OK;
}

// ---- resampling (resampling.rs) -------------------------------------------------------------------------------------

// local_basis (:188-214): false if no offset is longer than 1e-10 or none is off the first one's line
bool local_basis(const double* pts, int64_t n, V3 c, V3& u, V3& v)
{
    int64_t i = 0;
    for (; i < n; ++i) {
        const V3 off = sub(at(pts, i), c);
        const double l = norm(off);
        if (l > 1e-10) { u = dvs(off, l); break; }
    }
    if (i == n) return false;
    for (int64_t k = 0; k < n; ++k) {
        const V3 cr = cross(u, sub(at(pts, k), c));
        const double l = norm(cr);
        if (l > 1e-10) {
            const V3 nrm = dvs(cr, l);
            const V3 w = cross(nrm, u);
            v = dvs(w, norm(w));
            return true;
        }
    }
    return false;
}

// has_full_angular_coverage (:40-66)
bool full_coverage(const double* pts, int64_t n, V3 c)
{
    if (n < 4) return false;
    V3 u, v;
    if (!local_basis(pts, n, c, u, v)) return false;
    bool q[4] = {false, false, false, false};
    for (int64_t i = 0; i < n; ++i) {
        const V3 off = sub(at(pts, i), c);
        const bool pu = dot(off, u) >= 0.0, pv = dot(off, v) >= 0.0;
        q[pu ? (pv ? 0 : 3) : (pv ? 1 : 2)] = true;
    }
    return q[0] && q[1] && q[2] && q[3];
}

// catmull_rom (:216-229), in the written order
inline V3 catmull_rom(V3 p, V3 c, V3 n, V3 a, double t)
{
    const double t2 = t * t, t3 = t2 * t;
    const V3 mp = mul(p, -1.0);
    const V3 A = mul(c, 2.0);
    const V3 B = mul(add(mp, n), t);
    const V3 Cc = mul(sub(add(sub(mul(p, 2.0), mul(c, 5.0)), mul(n, 4.0)), a), t2);
    const V3 D = mul(add(sub(add(mp, mul(c, 3.0)), mul(n, 3.0)), a), t3);
    return mul(add(add(add(A, B), Cc), D), 0.5);
}

// resample_spline (:69-90) for one contour of n points around centroid c: 1 = written (n_points xyz triples), 0 = None,
// MM_ERR_INVALID on a NaN angle (a panic of the stable sort's partial_cmp().unwrap() in the reference, :107)
int resample(const double* pts, int64_t n, V3 c, int64_t n_points, double* out)
{
    if (n_points < 2 || n < 3) return 0;
    V3 u, v;
    if (!local_basis(pts, n, c, u, v)) return 0;
    std::vector<double> ang((size_t)n);                                           // sort_by_angle (:93-109)
    std::vector<int64_t> ord((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const V3 off = sub(at(pts, i), c);
        ang[(size_t)i] = std::atan2(dot(off, v), dot(off, u));
        if (std::isnan(ang[(size_t)i])) return set_error(MM_ERR_INVALID, "discretize: NaN angle in a contour (a panic in the reference)");
        ord[(size_t)i] = i;
    }
    std::stable_sort(ord.begin(), ord.end(), [&](int64_t a, int64_t b) { return ang[(size_t)a] < ang[(size_t)b]; });
    constexpr int kSeg = 32;                                                      // sample_closed_spline (:112-127)
    std::vector<V3> curve;
    curve.reserve((size_t)n * kSeg + 1);
    for (int64_t s = 0; s < n; ++s) {
        const V3 p = at(pts, ord[(size_t)((s + n - 1) % n)]), q = at(pts, ord[(size_t)s]);
        const V3 r = at(pts, ord[(size_t)((s + 1) % n)]), w = at(pts, ord[(size_t)((s + 2) % n)]);
        for (int k = 0; k < kSeg; ++k) curve.push_back(catmull_rom(p, q, r, w, (double)k / (double)kSeg));
    }
    curve.push_back(curve[0]);
    std::vector<double> arc(curve.size());                                        // cumulative_arc_lengths (:130-136)
    arc[0] = 0.0;
    for (size_t i = 1; i < curve.size(); ++i) arc[i] = arc[i - 1] + norm(sub(curve[i], curve[i - 1]));
    const double total = arc.back();
    if (total < 1e-10) return 0;
    const double step = total / (double)n_points;                                 // uniform_resample (:139-160)
    for (int64_t i = 0; i < n_points; ++i) {
        const double target = (double)i * step;
        size_t seg = (size_t)(std::lower_bound(arc.begin(), arc.end(), target) - arc.begin());   // partition_point(s < target)
        seg = seg == 0 ? 0 : seg - 1;
        seg = std::min(seg, curve.size() - 2);
        const double s0 = arc[seg], s1 = arc[seg + 1];
        const double f = std::fabs(s1 - s0) < 1e-12 ? 0.0 : (target - s0) / (s1 - s0);
        const V3 o = add(mul(curve[seg], 1.0 - f), mul(curve[seg + 1], f));
        out[3 * i] = o.x; out[3 * i + 1] = o.y; out[3 * i + 2] = o.z;
    }
    return 1;
}

// ---- device pass ----------------------------------------------------------------------------------------------------

// nearest anchor and plane projection of every point of every job (voronoi_partition, projecting.rs:62-104).
// pt_off / a_off: n_jobs + 1 offsets into pts (xyz) and anc (6 doubles each).  idx = -1 and proj = p where a job has
// no anchor (the reference drops such points).
int nearest_project(Engine* e, int n_jobs, const int64_t* pt_off, const double* pts, const int64_t* a_off,
                    const double* anc, int32_t* idx, double* proj)
{
    const int64_t NP = pt_off[n_jobs], NA = a_off[n_jobs];
    if (NP == 0) return MM_OK;
    if (NP > INT32_MAX / 4 || NA > INT32_MAX / 8)
        return set_error(MM_ERR_TOO_LARGE, "discretize: too many points or anchors for one pass");
    std::vector<SliceJob> jobs((size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
        const int64_t np = pt_off[j + 1] - pt_off[j], na = a_off[j + 1] - a_off[j];
        jobs[(size_t)j] = SliceJob{(int32_t)pt_off[j], (int32_t)np, (int32_t)a_off[j], (int32_t)na};
        if (na) continue;
        std::fill(idx + pt_off[j], idx + pt_off[j + 1], -1);
        std::memcpy(proj + 3 * pt_off[j], pts + 3 * pt_off[j], (size_t)np * 24);
    }
    return nearest_pass(e, jobs, pt_off, pts, a_off, 6, [&](double* ha) { if (NA) std::memcpy(ha, anc, (size_t)NA * 48); },
                        slice_block_points(), launch_slice_nearest, "nearest-anchor launch", idx, proj);
}

}  // namespace
}  // namespace mm

using namespace mm;

extern "C" {

int64_t mm_slice_anchor_count(const mm_clpoint* cl, int64_t ncl, uint32_t branch_id, double step_size)
{
    if (ncl < 0 || (ncl > 0 && !cl)) return set_error(MM_ERR_INVALID, "mm_slice_anchor_count: bad arguments");
    int64_t k = 0;
    const int rc = slice_anchors(cl, ncl, branch_id, step_size, nullptr, k);
    return rc ? rc : k;
}

int mm_nearest_anchor_project(mm_engine* h, int n_jobs, const int64_t* pt_off, const double* pts_xyz,
                              const int64_t* anchor_off, const double* anchors, int32_t* anchor_idx, double* proj_xyz)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (n_jobs < 0 || (n_jobs > 0 && (!pt_off || !anchor_off)))
        return set_error(MM_ERR_INVALID, "mm_nearest_anchor_project: bad arguments");
    if (n_jobs == 0) return MM_OK;
    if (!offsets_ok(pt_off, n_jobs) || !offsets_ok(anchor_off, n_jobs))
        return set_error(MM_ERR_INVALID, "mm_nearest_anchor_project: offsets must start at 0 and not decrease");
    if ((pt_off[n_jobs] > 0 && (!pts_xyz || !anchor_idx || !proj_xyz)) || (anchor_off[n_jobs] > 0 && !anchors))
        return set_error(MM_ERR_INVALID, "mm_nearest_anchor_project: bad arguments");
    return nearest_project(e, n_jobs, pt_off, pts_xyz, anchor_off, anchors, anchor_idx, proj_xyz);
}

int mm_resample_closed_contour(const double* pts, int64_t n, const double centroid[3], int64_t n_points, double* out)
{
    if (n < 0 || (n > 0 && !pts) || !centroid || !out || n_points < 2 || n_points > MM_DISCRETIZE_MAX_POINTS)
        return set_error(MM_ERR_INVALID, "mm_resample_closed_contour: bad arguments");
    return resample(pts, n, V3{centroid[0], centroid[1], centroid[2]}, n_points, out);
}

int mm_discretize_vessel_batch(mm_engine* h, int n_jobs, const mm_clpoint* cl, const int64_t* cl_off,
                               const uint32_t* branch_id, const double* pts_xyz, const int64_t* pt_off, double step_size,
                               int64_t n_points, const int64_t* out_off, int64_t* n_contours, int32_t* ids,
                               double* centroids_xyz, double* out_xyz)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (n_jobs < 0 || (n_jobs > 0 && (!cl_off || !branch_id || !pt_off || !out_off || !n_contours)))
        return set_error(MM_ERR_INVALID, "mm_discretize_vessel_batch: bad arguments");
    if (n_points < 2 || n_points > MM_DISCRETIZE_MAX_POINTS)
        return set_error(MM_ERR_INVALID, "mm_discretize_vessel_batch: n_points must be in [2, MM_DISCRETIZE_MAX_POINTS]");
    if (!(step_size > 0.0) || !std::isfinite(step_size))
        return set_error(MM_ERR_INVALID, "mm_discretize_vessel_batch: step_size must be finite and > 0");
    if (n_jobs == 0) return MM_OK;
    if (!offsets_ok(cl_off, n_jobs) || !offsets_ok(pt_off, n_jobs) || !offsets_ok(out_off, n_jobs))
        return set_error(MM_ERR_INVALID, "mm_discretize_vessel_batch: offsets must start at 0 and not decrease");
    if ((cl_off[n_jobs] > 0 && !cl) || (pt_off[n_jobs] > 0 && !pts_xyz) ||
        (out_off[n_jobs] > 0 && (!ids || !centroids_xyz || !out_xyz)))
        return set_error(MM_ERR_INVALID, "mm_discretize_vessel_batch: bad arguments");
    // anchors of every job (walk_centerline_slices, projecting.rs:19-39)
    std::vector<double> anc;
    std::vector<int64_t> a_off((size_t)n_jobs + 1, 0);
    for (int j = 0; j < n_jobs; ++j) {
        std::vector<double> aj;
        int64_t k = 0;
        if ((rc = slice_anchors(cl + cl_off[j], cl_off[j + 1] - cl_off[j], branch_id[j], step_size, &aj, k))) return rc;
        if (k > out_off[j + 1] - out_off[j])
            return set_error(MM_ERR_INVALID, "mm_discretize_vessel_batch: out_off gives a job fewer slots than its anchors "
                                             "(size them with mm_slice_anchor_count)");
        anc.insert(anc.end(), aj.begin(), aj.end());
        a_off[(size_t)j + 1] = a_off[(size_t)j] + k;
    }
    const int64_t NP = pt_off[n_jobs];
    std::vector<int32_t> idx((size_t)NP);
    std::vector<double> proj((size_t)NP * 3);
    if ((rc = nearest_project(e, n_jobs, pt_off, pts_xyz, a_off.data(), anc.data(), idx.data(), proj.data()))) return rc;
    // buckets in input order (projecting.rs:90-99), then create_uniform_contours (resampling.rs:11-37) per job
    struct Item { int job; int64_t anchor, slot, b_lo, b_hi; };
    std::vector<Item> items;
    std::vector<int64_t> bstart((size_t)a_off[n_jobs] + 1, 0);
    std::vector<double> bucket((size_t)NP * 3);
    for (int j = 0; j < n_jobs; ++j) {
        const int64_t na = a_off[j + 1] - a_off[j], A = a_off[j];
        n_contours[j] = 0;
        if (na == 0) continue;
        for (int64_t i = pt_off[j]; i < pt_off[j + 1]; ++i) ++bstart[(size_t)(A + idx[i]) + 1];
        for (int64_t k = 0; k < na; ++k) bstart[(size_t)(A + k) + 1] += bstart[(size_t)(A + k)];
        std::vector<int64_t> fill(bstart.begin() + A, bstart.begin() + A + na);
        for (int64_t i = pt_off[j]; i < pt_off[j + 1]; ++i) {
            const int64_t b = fill[(size_t)idx[i]]++;
            std::memcpy(&bucket[(size_t)b * 3], &proj[(size_t)i * 3], 24);
        }
        std::vector<int64_t> ne;                                                  // non-empty buckets
        for (int64_t k = 0; k < na; ++k)
            if (bstart[(size_t)(A + k) + 1] > bstart[(size_t)(A + k)]) ne.push_back(k);
        auto cov = [&](int64_t k) {
            const double* a = &anc[(size_t)(A + k) * 6];
            const int64_t lo = bstart[(size_t)(A + k)], hi = bstart[(size_t)(A + k) + 1];
            return full_coverage(&bucket[(size_t)lo * 3], hi - lo, V3{a[0], a[1], a[2]});
        };
        size_t start = 0, end = ne.size();                                        // :19-29 unwrap_or(0) / unwrap_or(len)
        while (start < ne.size() && !cov(ne[start])) ++start;
        if (start == ne.size()) start = 0;
        else { end = ne.size(); while (!cov(ne[end - 1])) --end; }
        for (size_t q = start; q < end; ++q) {
            const int64_t k = ne[q];
            items.push_back(Item{j, k, out_off[j] + (int64_t)(q - start), bstart[(size_t)(A + k)], bstart[(size_t)(A + k) + 1]});
        }
    }
    // resample every kept contour into its slot of the trimmed list; then close the gaps of the contours that gave None
    std::vector<int> res(items.size(), 0);
    WorkerPool::instance().parallel_for((int)items.size(), [&](int t) {
        const Item& it = items[(size_t)t];
        const double* a = &anc[(size_t)(a_off[it.job] + it.anchor) * 6];
        res[(size_t)t] = resample(&bucket[(size_t)it.b_lo * 3], it.b_hi - it.b_lo, V3{a[0], a[1], a[2]}, n_points,
                                  out_xyz + (size_t)it.slot * (size_t)n_points * 3);
    });
    for (size_t t = 0; t < items.size(); ++t)
        if (res[t] < 0) return set_error(MM_ERR_INVALID, "discretize: NaN angle in a contour (a panic in the reference)");
    for (size_t t = 0; t < items.size(); ++t) {
        if (res[t] != 1) continue;
        const Item& it = items[t];
        const int64_t dst = out_off[it.job] + n_contours[it.job]++;
        if (dst != it.slot)
            std::memmove(out_xyz + (size_t)dst * (size_t)n_points * 3, out_xyz + (size_t)it.slot * (size_t)n_points * 3,
                         (size_t)n_points * 24);
        ids[dst] = (int32_t)it.anchor;
        const double* a = &anc[(size_t)(a_off[it.job] + it.anchor) * 6];
        centroids_xyz[3 * dst] = a[0]; centroids_xyz[3 * dst + 1] = a[1]; centroids_xyz[3 * dst + 2] = a[2];
    }
    return MM_OK;
}

}  // extern "C"
