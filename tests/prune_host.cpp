// csrc/mm_prune.h on the CPU, no GPU, no HIP and no engine: the slab permutation on empty, single, equal, NaN, infinite
// and overflowing keys and on two cells of 1025 keys (stability across both radix passes), the box on NaN coordinates,
// box_lb2 on touching, overlapping and disjoint boxes (with slack 0.0: the bits of the four-operation formula written
// out here), and the nearest-first order on tied bounds.
#include <algorithm>
#include <array>
#include <cstdio>
#include <cstring>
#include <limits>
#include <numeric>

#include "mm_prune.h"

using namespace mm;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static const double kNaN = std::numeric_limits<double>::quiet_NaN(), kInf = std::numeric_limits<double>::infinity();

static unsigned long long bits(double v) { unsigned long long b; std::memcpy(&b, &v, 8); return b; }

static std::vector<int32_t> order_of(const std::vector<double>& key)
{
    std::vector<int32_t> order{7, 7, 7};   // whatever it held is replaced
    slab_permutation(key, order);
    return order;
}

static bool identity(const std::vector<int32_t>& o, size_t n)
{
    if (o.size() != n) return false;
    for (size_t i = 0; i < n; ++i) if (o[i] != (int32_t)i) return false;
    return true;
}

static int permutation()
{
    CHECK(order_of({}).empty());
    CHECK(identity(order_of({4.5}), 1));
    CHECK(identity(order_of({kNaN}), 1));
    CHECK(identity(order_of(std::vector<double>(777, -3.25)), 777));              // equal keys: sc = 0
    CHECK(identity(order_of(std::vector<double>(5, kNaN)), 5));                   // lo = DBL_MAX > hi = -DBL_MAX
    // NaN keys are ignored by lo / hi and land in cell 0, by index among the keys of that cell
    CHECK((order_of({3.0, kNaN, 1.0, 2.0, kNaN}) == std::vector<int32_t>{1, 2, 4, 3, 0}));
    // a range that overflows, and infinite keys: hi > lo holds but 1048575 / inf = 0 -- the identity
    CHECK(identity(order_of({DBL_MAX, -DBL_MAX, 0.0, 1.0}), 4));
    CHECK(identity(order_of({1.0, kInf, 0.0}), 3));
    CHECK(identity(order_of({1.0, -kInf, 0.0, kInf, kNaN}), 5));
    CHECK(identity(order_of({kInf, kInf}), 2));
    // two cells (the lowest and the highest: they differ in both 10-bit digits), 1025 keys: each cell keeps index order
    std::vector<double> key(1025);
    std::vector<int32_t> want;
    for (size_t i = 0; i < key.size(); ++i) key[i] = (i * 7 % 3 == 0) ? 1.0 : 0.0;
    for (int pass = 0; pass < 2; ++pass)
        for (size_t i = 0; i < key.size(); ++i) if ((key[i] == 1.0) == (pass == 1)) want.push_back((int32_t)i);
    CHECK(order_of(key) == want);
    // many cells, many repeats: a stable sort by the cell, restated here
    key.resize(5000);
    unsigned long long x = 12345;
    for (double& k : key) { x = x * 6364136223846793005ull + 1442695040888963407ull; k = (double)((x >> 33) % 1900) * 0.37 - 211.0; }
    const double lo = *std::min_element(key.begin(), key.end()), hi = *std::max_element(key.begin(), key.end());
    std::vector<uint32_t> cell(key.size());
    for (size_t i = 0; i < key.size(); ++i) {
        const double t = (key[i] - lo) * (1048575.0 / (hi - lo));
        cell[i] = t > 0.0 ? (t < 1048575.0 ? (uint32_t)t : 1048575u) : 0u;
    }
    want.resize(key.size());
    std::iota(want.begin(), want.end(), 0);
    std::stable_sort(want.begin(), want.end(), [&](int32_t a, int32_t b) { return cell[(size_t)a] < cell[(size_t)b]; });
    CHECK(order_of(key) == want);
    return 0;
}

static Box3 box_of(std::initializer_list<std::array<double, 3>> pts)
{
    Box3 b;
    for (const auto& p : pts) b.add(p.data());
    return b;
}

static int boxes()
{
    Box3 b;
    CHECK(b.lo[0] == DBL_MAX && b.lo[2] == DBL_MAX && b.hi[0] == -DBL_MAX && b.hi[2] == -DBL_MAX);
    b = box_of({{kNaN, kNaN, kNaN}, {kNaN, kNaN, kNaN}});                         // nothing but NaN: as empty
    for (int a = 0; a < 3; ++a) CHECK(b.lo[a] == DBL_MAX && b.hi[a] == -DBL_MAX);
    b = box_of({{1.0, kNaN, -2.0}, {kNaN, 5.0, 3.0}, {-4.0, 6.0, kNaN}});         // a NaN coordinate is ignored
    double six[6];
    static_assert(sizeof(b) == sizeof(six), "six doubles");
    std::memcpy(six, &b, sizeof(six));                                            // lo xyz, hi xyz
    const double want[6] = {-4.0, 5.0, -2.0, 1.0, 6.0, 3.0};
    for (int k = 0; k < 6; ++k) CHECK(six[k] == want[k]);
    CHECK(b.largest() == 6.0 && b.longest_axis() == 0 && box_of({{0, 0, 0}, {1, 1, 1}}).longest_axis() == 0);
    CHECK(box_of({{0, 0, 0}, {1, 2, 2}}).longest_axis() == 1 && box_of({{0, 0, -9}, {1, 2, 2}}).longest_axis() == 2);
    CHECK(box_of({{-7.5, 1, 2}}).largest() == 7.5);
    return 0;
}

// the bound as the nearest-neighbour path computed it: four operations a gap, no slack anywhere
static double formula(const Box3& a, const Box3& b)
{
    double s = 0.0;
    for (int ax = 0; ax < 3; ++ax) {
        const double gap = std::max(0.0, std::max(a.lo[ax] - b.hi[ax], b.lo[ax] - a.hi[ax]));
        s += gap * gap;
    }
    return s * (1.0 - 1e-12);
}

static int bounds()
{
    const Box3 unit = box_of({{0, 0, 0}, {1, 1, 1}});
    const Box3 touching = box_of({{1, 0, 0}, {2, 1, 1}}), overlapping = box_of({{0.5, 0.5, 0.5}, {3, 3, 3}});
    const Box3 disjoint = box_of({{3, 5, -2.5}, {4, 6, -2}}), nothing, far = box_of({{1e308, -1e308, 0.1}});
    const Box3 inf = box_of({{kInf, -kInf, 0.3}, {2, 2, 2}}), tiny = box_of({{1.0 + DBL_EPSILON, 1e-300, -0.0}});
    CHECK(bits(box_lb2(unit, touching, 0.0)) == bits(0.0) && bits(box_lb2(unit, overlapping, 0.0)) == bits(0.0));
    CHECK(box_lb2(unit, disjoint, 0.0) == (4.0 + 16.0 + 4.0) * (1.0 - 1e-12));
    const Box3 all[] = {unit, touching, overlapping, disjoint, nothing, far, inf, tiny};
    for (const Box3& a : all)
        for (const Box3& b : all) {
            CHECK(bits(box_lb2(a, b, 0.0)) == bits(formula(a, b)));                // - 0.0 changes no bit
            CHECK(bits(box_lb2(a, b, 0.0)) == bits(box_lb2(b, a, 0.0)));
            CHECK(!(box_lb2(a, b, 0.25) > box_lb2(a, b, 0.0)));                    // slack only lowers a bound
        }
    CHECK(box_lb2(unit, disjoint, 0.5) == (2.25 + 12.25 + 2.25) * (1.0 - 1e-12)); // gaps 2, 4, 2 narrowed by 0.5
    CHECK(bits(box_lb2(unit, disjoint, 4.0)) == bits(0.0));                        // never below 0
    return 0;
}

static int order()
{
    std::vector<std::pair<double, int32_t>> cand(9);
    const double lb2[5] = {5.0, 0.0, 0.0, 3.0, 0.0};
    nearest_first(5, [&](int64_t c) { return lb2[c]; }, cand);
    const std::vector<std::pair<double, int32_t>> want{{0.0, 1}, {0.0, 2}, {0.0, 4}, {3.0, 3}, {5.0, 0}};
    CHECK(cand == want);                                                          // tied bounds: lowest chunk first
    nearest_first(1, [&](int64_t) { return kInf; }, cand);
    CHECK(cand.size() == 1 && cand[0].first == kInf && cand[0].second == 0);
    return 0;
}

int main()
{
    if (permutation() || boxes() || bounds() || order()) return 1;
    std::printf("prune_host OK\n");
    return 0;
}
