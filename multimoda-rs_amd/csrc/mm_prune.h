// mm_prune.h -- the host half of the pruned exact-f64 searches (nearest neighbour: mm_ccta.cpp / mm_nn_kernels.hip; point
// to triangle: mm_surface.cpp / mm_tri_kernels.hip): the slab order both sides are staged in, the boxes of their groups,
// the lower bound lb2 every (query block, chunk) item carries, and the order the items run in.  The device half is
// mm_prune_device.h; the argument that pruning returns the bits of a full scan is DESIGN.md 4.20.  Plain C++17, no HIP
// and no engine header: tests/prune_host.cpp includes it on its own.  Box3, box_lb2 and tri_slack are MM_HD: a HIP
// compiler also builds them for the device, where the mesh relaxation (mm_relax_kernels.hip) refreshes the bounds of
// queries that move -- one formula on both sides.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MM_HD __host__ __device__
#else
#define MM_HD
#endif

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace mm {

// Bounding box of the points added so far.  std::min / std::max with the running value first: a NaN coordinate is
// ignored, and a group of nothing but NaN keeps (DBL_MAX, -DBL_MAX).  Six doubles: lo xyz, hi xyz.
struct Box3 {
    double lo[3] = {DBL_MAX, DBL_MAX, DBL_MAX}, hi[3] = {-DBL_MAX, -DBL_MAX, -DBL_MAX};
    MM_HD void add(const double* p) { for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], p[a]); hi[a] = std::max(hi[a], p[a]); } }
    MM_HD double largest() const { double m = 0.0; for (int a = 0; a < 3; ++a) m = std::max(m, std::max(std::fabs(lo[a]), std::fabs(hi[a]))); return m; }
    int longest_axis() const { int ax = 0; for (int a = 1; a < 3; ++a) if (hi[a] - lo[a] > hi[ax] - lo[ax]) ax = a; return ax; }
};
static_assert(sizeof(Box3) == 48, "Box3 is six doubles");

// Slab order: indices 0 .. n-1 by their key quantised to 20 bits of the keys' range [lo, hi], equal cells by index (a
// stable LSD radix sort, two passes of 10 bits, where a full sort took most of a call's host time).  Any permutation
// gives the same results; this one makes runs of consecutive staged elements slabs across the key's axis.  lo and hi
// are taken with the running value first: NaN keys are ignored there and land in cell 0 (the clamp is false for a NaN
// on both sides).  sc = 0, the identity order, for no key, equal keys or nothing but NaN (hi > lo is false), and for a
// range that overflows or an infinite key (1048575 / inf = 0, and (key - lo) * 0 is 0 or NaN).
// Nearest neighbour tested `hi > lo` on the box of Set3::at along the axis: these lo and hi; its keys may be NaN or
// +-inf.  Point to triangle tested `hi - lo > 0` on std::minmax_element.  Its input is finite, so its keys are never NaN
// (a corner sum overflows to one infinity at most), minmax_element finds the same lo and hi (up to the sign of a zero,
// which the cells do not see), and without NaN `hi - lo > 0` is `hi > lo`: distinct doubles never subtract to zero,
// inf - finite is inf, inf - inf is NaN and fails both.  One test serves both callers bit for bit.
inline void slab_permutation(const std::vector<double>& key, std::vector<int32_t>& order)
{
    const size_t n = key.size();
    order.resize(n);
    double lo = DBL_MAX, hi = -DBL_MAX;
    for (size_t i = 0; i < n; ++i) { lo = std::min(lo, key[i]); hi = std::max(hi, key[i]); }
    const double sc = hi > lo ? 1048575.0 / (hi - lo) : 0.0;
    std::vector<uint32_t> cell(n), cell2(n);
    std::vector<int32_t> idx2(n);
    for (size_t i = 0; i < n; ++i) {
        const double t = (key[i] - lo) * sc;
        cell[i] = t > 0.0 ? (t < 1048575.0 ? (uint32_t)t : 1048575u) : 0u;   // NaN-safe clamp
        order[i] = (int32_t)i;
    }
    for (int sh = 0; sh < 20; sh += 10) {
        uint32_t cnt[1025] = {0};
        for (size_t i = 0; i < n; ++i) ++cnt[((cell[i] >> sh) & 1023u) + 1];
        for (int b = 0; b < 1024; ++b) cnt[b + 1] += cnt[b];
        for (size_t i = 0; i < n; ++i) {
            const uint32_t d = cnt[(cell[i] >> sh) & 1023u]++;
            cell2[d] = cell[i]; idx2[d] = order[i];
        }
        cell.swap(cell2); order.swap(idx2);
    }
}

// THE bound: a lower bound of every squared distance the device computes between an element inside a and one inside b.
// Per axis the gap between the boxes, narrowed by slack and clamped at 0; the squares summed x, y, z from 0.0; the sum
// shaved by 1e-12 so that the roundings of the device's own sum of squares can never fall below it.  Nearest neighbour
// compares points that lie in the boxes exactly: slack = 0.0, and subtracting +0.0 changes no double's bits (-0.0 and
// NaN included), nor what std::max then does with a NaN (tests/golden/prune_plans.json holds the bits from before the
// function was shared).  Point to triangle measures to a closest point that rounding may place a few ulp outside the
// triangle's box: it passes tri_slack (mm_surface.cpp).
MM_HD inline double box_lb2(const Box3& a, const Box3& b, double slack)
{
    double s = 0.0;
    for (int ax = 0; ax < 3; ++ax) {
        const double gap = std::max(0.0, std::max(a.lo[ax] - b.hi[ax], b.lo[ax] - a.hi[ax]) - slack);
        s += gap * gap;
    }
    return s * (1.0 - 1e-12);
}

// The slack of the bound between a query block q and a chunk's corners c, point to triangle.  The closest point the rule
// computes, u + e t or (a + ab v) + ac w with factors that rounding keeps within a few ulp of [0, 1], lies within a few
// ulp of the largest coordinate of the triangle's own box, hence of the chunk's: each gap is narrowed by 64 such ulp
// (DESIGN 4.19).
MM_HD inline double tri_slack(const Box3& q, const Box3& c) { return 64.0 * DBL_EPSILON * std::max(q.largest(), c.largest()); }

// Nearest chunks first: (lb2, chunk) of a query block against chunks 0 .. nch-1, ascending, ties by chunk.  cand[0] is
// the block's item of pass A -- it runs unchecked and tightens the minima the others are checked against -- and
// cand[1 ..] its items of pass B, in this order.
template <class Bound>
inline void nearest_first(int64_t nch, Bound lb2_of_chunk, std::vector<std::pair<double, int32_t>>& cand)
{
    cand.resize((size_t)nch);
    for (int64_t c = 0; c < nch; ++c) cand[(size_t)c] = {lb2_of_chunk(c), (int32_t)c};
    std::sort(cand.begin(), cand.end());
}

}  // namespace mm
