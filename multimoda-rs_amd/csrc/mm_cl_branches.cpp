// mm_cl_branches.cpp -- the branch structure of a centerline (include/mm_centerline.h): finding the branches of a
// centerline written segment after segment, ordering, orienting, trimming, splitting, merging and smoothing them.
// Host f64 in the reference's operation order (the file is built with -ffp-contract=off).  Reference:
// src/types/native/centerline.rs:64-937 (lines cited per function).
//
// A branch is a maximal run of consecutive points with one branch_id: the reference's branch_start_indices are the
// first indices of these runs for every centerline it builds (rebuild_from_branches numbers the runs 0, 1, ...), and
// mm_clpoint carries no separate list.  ContourPoint.point_index is the position in the array.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <map>
#include <vector>

#include "../../include/mm_centerline.h"
#include "mm_engine.h"

namespace mm {
namespace {

using Branch = std::vector<mm_clpoint>;

// Point3D::distance_to (types/native.rs:27-32)
inline double dist(const mm_clpoint& a, const mm_clpoint& b)
{
    const double dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
    return std::sqrt(dx * dx + dy * dy + dz * dz);
}

// branches_as_vecs (:394-407)
std::vector<Branch> branches_of(const mm_clpoint* cl, int64_t n)
{
    std::vector<Branch> out;
    for (int64_t i = 0; i < n; ++i) {
        if (i == 0 || cl[i].branch_id != cl[i - 1].branch_id) out.emplace_back();
        out.back().push_back(cl[i]);
    }
    return out;
}

// recompute_tangents (:377-391): normalised forward differences inside a branch (a zero difference divides by zero,
// as nalgebra's normalize does); the last point of a branch repeats its predecessor's; a lone point gets zero
void recompute_tangents(mm_clpoint* p, int64_t n)
{
    for (int64_t i = 0; i < n; ++i) {
        if (i + 1 < n && p[i].branch_id == p[i + 1].branch_id) {
            const double dx = p[i + 1].x - p[i].x, dy = p[i + 1].y - p[i].y, dz = p[i + 1].z - p[i].z;
            const double nn = std::sqrt(dx * dx + dy * dy + dz * dz);
            p[i].tx = dx / nn; p[i].ty = dy / nn; p[i].tz = dz / nn;
        } else if (i > 0 && p[i - 1].branch_id == p[i].branch_id) {
            p[i].tx = p[i - 1].tx; p[i].ty = p[i - 1].ty; p[i].tz = p[i - 1].tz;
        } else {
            p[i].tx = p[i].ty = p[i].tz = 0.0;
        }
    }
}

// rebuild_from_branches (:411-430): branch k gets id k; returns the number of points written
int64_t rebuild(const std::vector<Branch>& branches, mm_clpoint* out)
{
    int64_t k = 0;
    for (size_t b = 0; b < branches.size(); ++b)
        for (mm_clpoint pt : branches[b]) { pt.branch_id = (uint32_t)b; pt.pad_ = 0; out[k++] = pt; }
    recompute_tangents(out, k);
    return k;
}

int64_t copy_unchanged(const mm_clpoint* cl, int64_t n, mm_clpoint* out)
{
    if (n > 0) std::memcpy(out, cl, (size_t)n * sizeof(mm_clpoint));
    return n;
}

// sort_branches_by_length (:558-560): descending number of points, ties keep their order
void sort_by_length(std::vector<Branch>& b)
{
    std::stable_sort(b.begin(), b.end(), [](const Branch& x, const Branch& y) { return x.size() > y.size(); });
}

// ---- calculate_branches (:78-155) ----------------------------------------------------------------------------------

// p95_consecutive_spacing (:325-339)
double p95_spacing(const mm_clpoint* p, int64_t n)
{
    if (n < 2) return 1.0;
    std::vector<double> s((size_t)n - 1);
    for (int64_t i = 1; i < n; ++i) s[(size_t)i - 1] = dist(p[i - 1], p[i]);
    std::sort(s.begin(), s.end());
    return s[s.size() * 95 / 100];
}

using Adj = std::vector<std::vector<int64_t>>;

// build_sparse_tree_adjacency (:158-207): consecutive points within the threshold; between every two segments one edge at
// their closest pair (strict <: the first minimum in (pi, pj) order) if that is within the threshold
void sparse_tree(const mm_clpoint* p, int64_t n, const std::vector<int64_t>& seg, double threshold, Adj& adj)
{
    adj.assign((size_t)n, {});
    for (int64_t i = 1; i < n; ++i)
        if (dist(p[i - 1], p[i]) <= threshold) { adj[(size_t)i - 1].push_back(i); adj[(size_t)i].push_back(i - 1); }
    const size_t ns = seg.size() - 1;
    for (size_t si = 0; si < ns; ++si)
        for (size_t sj = si + 1; sj < ns; ++sj) {
            double best = INFINITY;
            int64_t bi = seg[si], bj = seg[sj];
            for (int64_t pi = seg[si]; pi < seg[si + 1]; ++pi)
                for (int64_t pj = seg[sj]; pj < seg[sj + 1]; ++pj) {
                    const double d = dist(p[pi], p[pj]);
                    if (d < best) { best = d; bi = pi; bj = pj; }
                }
            if (best <= threshold) { adj[(size_t)bi].push_back(bj); adj[(size_t)bj].push_back(bi); }
        }
}

// bfs_farthest (:253-281): arc length from start over the tree; the farthest node (strict >: the first one reached)
int64_t bfs_farthest(const mm_clpoint* p, const Adj& adj, int64_t start, std::vector<int64_t>& prev)
{
    const size_t n = adj.size();
    std::vector<double> d(n, INFINITY);
    prev.assign(n, -1);
    std::deque<int64_t> q;
    d[(size_t)start] = 0.0;
    q.push_back(start);
    int64_t far = start;
    while (!q.empty()) {
        const int64_t u = q.front();
        q.pop_front();
        for (int64_t v : adj[(size_t)u])
            if (std::isinf(d[(size_t)v])) {
                d[(size_t)v] = d[(size_t)u] + dist(p[u], p[v]);
                prev[(size_t)v] = u;
                q.push_back(v);
                if (d[(size_t)v] > d[(size_t)far]) far = v;
            }
    }
    return far;
}

// order_chain (:342-371): the component walked from its first point with at most one neighbour inside it; points the
// walk does not reach follow in component order
std::vector<int64_t> order_chain(const std::vector<int64_t>& comp, const Adj& adj, std::vector<int32_t>& mark, int32_t tag)
{
    // mark[v]: tag = in the component, tag + 1 = in the component and seen (tags of different components differ by 2)
    for (int64_t v : comp) mark[(size_t)v] = tag;
    auto inside = [&](int64_t v) { return mark[(size_t)v] == tag || mark[(size_t)v] == tag + 1; };
    int64_t start = comp[0];
    for (int64_t v : comp) {
        int deg = 0;
        for (int64_t nb : adj[(size_t)v]) deg += inside(nb);
        if (deg <= 1) { start = v; break; }
    }
    std::vector<int64_t> ordered;
    ordered.reserve(comp.size());
    for (int64_t cur = start;;) {
        ordered.push_back(cur);
        mark[(size_t)cur] = tag + 1;
        int64_t next = -1;
        for (int64_t nb : adj[(size_t)cur])
            if (mark[(size_t)nb] == tag) { next = nb; break; }
        if (next < 0) break;
        cur = next;
    }
    for (int64_t v : comp)
        if (mark[(size_t)v] == tag) ordered.push_back(v);
    return ordered;
}

int64_t calculate_branches(const mm_clpoint* p, int64_t n, double tol, mm_clpoint* out)
{
    constexpr size_t kMinBranch = 5;
    const double threshold = p95_spacing(p, n) * tol;
    std::vector<int64_t> seg{0};
    for (int64_t i = 1; i < n; ++i)
        if (dist(p[i - 1], p[i]) > threshold) seg.push_back(i);
    seg.push_back(n);
    Adj adj;
    sparse_tree(p, n, seg, threshold, adj);

    // identify_components_with_bfs (:209-247): the tree diameter from point 0's farthest node, then the components of the rest
    std::vector<int64_t> prev;
    const int64_t a = bfs_farthest(p, adj, 0, prev);
    const int64_t b = bfs_farthest(p, adj, a, prev);
    std::vector<int64_t> main_path;
    for (int64_t cur = b;;) {                                                             // trace_path (:284-298)
        main_path.push_back(cur);
        if (cur == a || prev[(size_t)cur] < 0) break;
        cur = prev[(size_t)cur];
    }
    std::vector<uint8_t> visited((size_t)n, 0);
    for (int64_t v : main_path) visited[(size_t)v] = 1;
    std::vector<std::vector<int64_t>> sides;
    for (int64_t s = 0; s < n; ++s) {
        if (visited[(size_t)s]) continue;
        std::vector<int64_t> comp;
        std::deque<int64_t> q{s};
        visited[(size_t)s] = 1;
        while (!q.empty()) {
            const int64_t u = q.front();
            q.pop_front();
            comp.push_back(u);
            for (int64_t v : adj[(size_t)u])
                if (!visited[(size_t)v]) { visited[(size_t)v] = 1; q.push_back(v); }
        }
        if (comp.size() >= kMinBranch) sides.push_back(std::move(comp));                 // :106-115 smaller ones are artefacts
    }
    std::stable_sort(sides.begin(), sides.end(),                                          // :116
                     [](const std::vector<int64_t>& x, const std::vector<int64_t>& y) { return x.size() > y.size(); });
    int64_t k = 0;
    for (int64_t v : main_path) { out[k] = p[v]; out[k].branch_id = 0; out[k].pad_ = 0; ++k; }
    std::vector<int32_t> mark((size_t)n, 0);
    for (size_t s = 0; s < sides.size(); ++s)
        for (int64_t v : order_chain(sides[s], adj, mark, (int32_t)(2 * s + 1))) {
            out[k] = p[v]; out[k].branch_id = (uint32_t)(s + 1); out[k].pad_ = 0; ++k;
        }
    recompute_tangents(out, k);
    return k;
}

// ---- orientation (:562-670) ----------------------------------------------------------------------------------------

// should_reverse_by_max_z (:628-644): Iterator::max_by keeps the LAST of equal maxima, and a NaN compares Equal
bool reverse_by_max_z(const Branch& b)
{
    size_t best = 0;
    for (size_t i = 1; i < b.size(); ++i)
        if (!(b[best].z > b[i].z)) best = i;
    return best != 0;
}

// should_reverse_relative_to (:648-670): the last point is nearer to the reference (its nearest point) than the first
bool reverse_relative_to(const Branch& b, const mm_clpoint* ref, int64_t nref)
{
    if (b.empty() || nref <= 0) return false;
    double df = INFINITY, dl = INFINITY;
    for (int64_t i = 0; i < nref; ++i) df = std::fmin(df, dist(ref[i], b.front()));
    for (int64_t i = 0; i < nref; ++i) dl = std::fmin(dl, dist(ref[i], b.back()));
    return dl < df;
}

int64_t first_run(const mm_clpoint* cl, int64_t n)                                        // branch_0 (:618-625)
{
    int64_t e = n > 0 ? 1 : 0;
    while (e < n && cl[e].branch_id == cl[0].branch_id) ++e;
    return e;
}

bool bad(const mm_clpoint* cl, int64_t n, const void* out) { return n < 0 || (n > 0 && (!cl || !out)); }

}  // namespace

// recompute_tangents for the other files that build a centerline (mm_geodesic.cpp)
void cl_recompute_tangents(mm_clpoint* p, int64_t n) { recompute_tangents(p, n); }

}  // namespace mm

using namespace mm;

extern "C" {

int64_t mm_centerline_calculate_branches(const mm_clpoint* cl, int64_t n, double spacing_tolerance, mm_clpoint* out)
{
    if (bad(cl, n, out)) return set_error(MM_ERR_INVALID, "mm_centerline_calculate_branches: bad arguments");
    if (n == 0) return 0;                                                                  // :82-85
    if (n > INT32_MAX / 2) return set_error(MM_ERR_TOO_LARGE, "mm_centerline_calculate_branches: too many points");
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(cl[i].x) || !std::isfinite(cl[i].y) || !std::isfinite(cl[i].z))
            return set_error(MM_ERR_INVALID, "mm_centerline_calculate_branches: a coordinate is not finite");
    return calculate_branches(cl, n, spacing_tolerance, out);
}

int64_t mm_centerline_find_sharp_angles(const mm_clpoint* cl, int64_t n, uint32_t branch, double cos_threshold,
                                        int64_t* out_idx)
{
    if (bad(cl, n, out_idx)) return set_error(MM_ERR_INVALID, "mm_centerline_find_sharp_angles: bad arguments");
    int64_t start = 0, run = 0, k = 0;
    for (; start < n; ++run) {                                                            // :437-448 the branch-th run
        int64_t end = start + 1;
        while (end < n && cl[end].branch_id == cl[start].branch_id) ++end;
        if (run == (int64_t)branch) {
            for (int64_t i = start + 1; i + 1 < end; ++i) {                               // :450-465
                const double ax = cl[i - 1].x - cl[i].x, ay = cl[i - 1].y - cl[i].y, az = cl[i - 1].z - cl[i].z;
                const double bx = cl[i + 1].x - cl[i].x, by = cl[i + 1].y - cl[i].y, bz = cl[i + 1].z - cl[i].z;
                const double n1 = std::sqrt(ax * ax + ay * ay + az * az), n2 = std::sqrt(bx * bx + by * by + bz * bz);
                if (n1 < 1e-10 || n2 < 1e-10) continue;
                if ((ax * bx + ay * by + az * bz) / (n1 * n2) > cos_threshold) out_idx[k++] = i;
            }
            break;
        }
        start = end;
    }
    return k;
}

int64_t mm_centerline_split_branch(const mm_clpoint* cl, int64_t n, uint32_t branch, int64_t point_index, mm_clpoint* out)
{
    if (bad(cl, n, out)) return set_error(MM_ERR_INVALID, "mm_centerline_split_branch: bad arguments");
    std::vector<Branch> br = branches_of(cl, n);
    const size_t idx = branch;
    if (idx >= br.size()) return copy_unchanged(cl, n, out);                              // :477-479
    int64_t start = 0;
    for (size_t b = 0; b < idx; ++b) start += (int64_t)br[b].size();
    const int64_t end = start + (int64_t)br[idx].size();
    if (point_index < start || point_index >= end) return copy_unchanged(cl, n, out);     // :486-488
    const size_t local = (size_t)(point_index - start);
    if (local == 0 || local >= br[idx].size() - 1) return copy_unchanged(cl, n, out);     // :493-496
    const Branch whole = br[idx];
    br.erase(br.begin() + (std::ptrdiff_t)idx);
    br.emplace_back(whole.begin(), whole.begin() + (std::ptrdiff_t)local + 1);            // :498-501 both keep the split point
    br.emplace_back(whole.begin() + (std::ptrdiff_t)local, whole.end());
    sort_by_length(br);
    return rebuild(br, out);
}

int64_t mm_centerline_merge_branches(const mm_clpoint* cl, int64_t n, uint32_t branch_a, uint32_t branch_b, mm_clpoint* out)
{
    if (bad(cl, n, out)) return set_error(MM_ERR_INVALID, "mm_centerline_merge_branches: bad arguments");
    std::vector<Branch> br = branches_of(cl, n);
    const size_t ia = branch_a, ib = branch_b;
    if (ia == ib || ia >= br.size() || ib >= br.size()) return copy_unchanged(cl, n, out);   // :516-518
    const size_t lo = std::min(ia, ib), hi = std::max(ia, ib);
    Branch bh = br[hi], bl = br[lo];
    br.erase(br.begin() + (std::ptrdiff_t)hi);
    br.erase(br.begin() + (std::ptrdiff_t)lo);
    const double d_ll_hf = dist(bl.back(), bh.front()), d_ll_hl = dist(bl.back(), bh.back());   // :534-538
    const double d_lf_hf = dist(bl.front(), bh.front()), d_lf_hl = dist(bl.front(), bh.back());
    const double min_d = std::fmin(std::fmin(std::fmin(d_ll_hf, d_ll_hl), d_lf_hf), d_lf_hl);
    Branch merged;
    if (std::fabs(min_d - d_ll_hf) < 1e-12) {                                             // :540-548
        merged = bl; merged.insert(merged.end(), bh.begin(), bh.end());
    } else if (std::fabs(min_d - d_ll_hl) < 1e-12) {
        merged = bl; merged.insert(merged.end(), bh.rbegin(), bh.rend());
    } else if (std::fabs(min_d - d_lf_hf) < 1e-12) {
        merged.assign(bh.rbegin(), bh.rend()); merged.insert(merged.end(), bl.begin(), bl.end());
    } else {
        merged = bh; merged.insert(merged.end(), bl.begin(), bl.end());
    }
    br.push_back(std::move(merged));
    sort_by_length(br);
    return rebuild(br, out);
}

int64_t mm_centerline_orient_by_max_z(const mm_clpoint* cl, int64_t n, mm_clpoint* out)
{
    if (bad(cl, n, out)) return set_error(MM_ERR_INVALID, "mm_centerline_orient_by_max_z: bad arguments");
    if (n == 0) return 0;
    std::vector<Branch> br = branches_of(cl, n);
    if (reverse_by_max_z(br[0])) std::reverse(br[0].begin(), br[0].end());
    for (size_t b = 1; b < br.size(); ++b)                                                // :579-585 against branch 0 as it is now
        if (reverse_relative_to(br[b], br[0].data(), (int64_t)br[0].size())) std::reverse(br[b].begin(), br[b].end());
    return rebuild(br, out);
}

int64_t mm_centerline_orient_to_reference(const mm_clpoint* cl, int64_t n, const mm_clpoint* reference, int64_t n_ref,
                                          mm_clpoint* out)
{
    if (bad(cl, n, out) || n_ref < 0 || (n_ref > 0 && !reference))
        return set_error(MM_ERR_INVALID, "mm_centerline_orient_to_reference: bad arguments");
    if (n == 0) return 0;
    std::vector<Branch> br = branches_of(cl, n);
    const int64_t r0 = first_run(reference, n_ref);                                       // :605 the reference's branch 0 only
    for (Branch& b : br)
        if (reverse_relative_to(b, reference, r0)) std::reverse(b.begin(), b.end());
    return rebuild(br, out);
}

int64_t mm_centerline_remove_branch_overlap(const mm_clpoint* cl, int64_t n, mm_clpoint* out)
{
    if (bad(cl, n, out)) return set_error(MM_ERR_INVALID, "mm_centerline_remove_branch_overlap: bad arguments");
    if (n == 0) return 0;
    std::vector<Branch> br = branches_of(cl, n);
    double buffer = 1.0;                                                                  // mean_spacing (:304-319)
    if (br[0].size() >= 2) {
        double sum = 0.0;
        for (size_t i = 1; i < br[0].size(); ++i) sum += dist(br[0][i - 1], br[0][i]);
        buffer = sum / (double)(br[0].size() - 1);
    }
    const double buffer_sq = buffer * buffer;
    if (br.size() > 1) {                                                                  // remove_overlapping (:877-913)
        std::vector<mm_clpoint> known = br[0];
        for (size_t b = 1; b < br.size(); ++b) {
            Branch& cur = br[b];
            size_t j = 0;
            for (; j < cur.size(); ++j) {
                bool close = false;
                for (const mm_clpoint& m : known) {
                    const double dx = cur[j].x - m.x, dy = cur[j].y - m.y, dz = cur[j].z - m.z;
                    if (dx * dx + dy * dy + dz * dz <= buffer_sq) { close = true; break; }
                }
                if (!close) break;
            }
            if (j == cur.size()) cur.clear();                                             // wholly inside the buffer: dropped
            else if (j > 0) cur.erase(cur.begin(), cur.begin() + (std::ptrdiff_t)(j - 1));   // the last close point stays
            known.insert(known.end(), cur.begin(), cur.end());
        }
        br.erase(std::remove_if(br.begin(), br.end(), [](const Branch& x) { return x.empty(); }), br.end());
    }
    return rebuild(br, out);
}

int64_t mm_centerline_trim_start(const mm_clpoint* cl, int64_t n, double mm_len, mm_clpoint* out)
{
    if (bad(cl, n, out)) return set_error(MM_ERR_INVALID, "mm_centerline_trim_start: bad arguments");
    if (mm_len <= 0.0 || n == 0) return copy_unchanged(cl, n, out);                       // :699-701
    std::vector<Branch> br = branches_of(cl, n);
    Branch& b0 = br[0];
    if (b0.size() > 1) {                                                                  // remove_trailing_start (:917-937)
        double arc = 0.0;
        size_t trim = 0;
        for (size_t i = 1; i < b0.size(); ++i) {
            arc += dist(b0[i - 1], b0[i]);
            if (arc <= mm_len) trim = i;
            else break;
        }
        b0.erase(b0.begin(), b0.begin() + (std::ptrdiff_t)trim);
    }
    return rebuild(br, out);
}

int64_t mm_centerline_smooth(const mm_clpoint* cl, int64_t n, double sigma, mm_clpoint* out)
{
    if (bad(cl, n, out)) return set_error(MM_ERR_INVALID, "mm_centerline_smooth: bad arguments");
    copy_unchanged(cl, n, out);
    if (n == 0 || sigma < 1e-12) return n;                                                // :799-801
    std::map<uint32_t, std::vector<int64_t>> by_id;                                       // :810-817 the points of one id, in order
    for (int64_t i = 0; i < n; ++i) by_id[cl[i].branch_id].push_back(i);
    const double r3 = std::ceil(3.0 * sigma);                                             // :824, Rust's saturating cast
    const size_t radius = r3 != r3 || r3 <= 0.0 ? 0 : (r3 >= 9e18 ? SIZE_MAX : (size_t)r3);
    for (const auto& kv : by_id) {
        const std::vector<int64_t>& idx = kv.second;
        for (size_t li = 0; li < idx.size(); ++li) {
            const size_t sym = std::min(std::min(li, radius), idx.size() - 1 - li);      // :830 the same reach on both sides
            double wx = 0.0, wy = 0.0, wz = 0.0, wt = 0.0;
            for (size_t j = li - sym; j < li + sym + 1; ++j) {
                const double diff = (double)li - (double)j;
                const double w = std::exp(-0.5 * diff * diff / (sigma * sigma));
                const mm_clpoint& pt = cl[idx[j]];
                wx += w * pt.x; wy += w * pt.y; wz += w * pt.z; wt += w;
            }
            if (wt > 1e-12) {
                mm_clpoint& o = out[idx[li]];
                o.x = wx / wt; o.y = wy / wt; o.z = wz / wt;
            }
        }
    }
    recompute_tangents(out, n);
    return n;
}

}  // extern "C"
