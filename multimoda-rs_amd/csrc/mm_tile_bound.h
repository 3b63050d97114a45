// Tile bound of the culled matrix-pipe screen (k_screen_mx_cull, mm_kernels.hip): the layout of a set in tiles of 32 slots
// (mm_tile_slot_point: consecutive points, or the two runs of a split set tile by tile), a bounding circle per tile and a
// lower bound of the squared distance between any two points of two tiles.  Shared by the kernel and the host
// (mm_tile_bound_probe, the test hook that checks it against f64), so both run the same f32 operations.
//
// Units are the screen's scaled units (x = 2^e * coordinate, every point of the pair within 512 of the rotation centre:
// every coordinate, centre and radius below 2^10 in magnitude, every distance below 2^11).
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#if defined(__HIPCC__)
#define MM_TB_HD __host__ __device__
#else
#define MM_TB_HD
#endif

// square root: the hardware instruction on the device (1 ulp), the correctly rounded one on the host -- the slack of the
// bounds below covers either; a denormal argument flushed to 0 only lowers a gap, and a radius carries 2^-10 absolute
MM_TB_HD inline float mm_tb_sqrt(float x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_sqrtf(x);
#else
    return sqrtf(x);
#endif
}

// The point in slot j (>= 0) of a set of n points laid out in tiles of 32 slots.  main == 0: the points in order, the slots
// from n on duplicate the last point.  0 < main < n: the set is two runs, `main` points and then n - main (lumen and
// catheter of a search set), and each run starts a tile of its own: the first run fills ceil(main / 32) tiles, padded with
// its last point, the second run the slots behind them, padded with the set's last point.  Every point has a slot and a
// padding slot duplicates a point of its own run, so the multiset of values a screen takes minima over gains nothing new.
MM_TB_HD inline int mm_tile_slot_point(int j, int n, int main)
{
    if (main <= 0 || main >= n) return j < n ? j : n - 1;
    const int edge = ((main + 31) >> 5) << 5;
    if (j < edge) return j < main ? j : main - 1;
    const int k = j - edge, m = n - main;
    return main + (k < m ? k : m - 1);
}

// The split a set of n points in two runs (main, n - main) may take: it must add no tile.  Else 0 (no split).
MM_TB_HD inline int mm_tile_split_main(int n, int main)
{
    if (main <= 0 || main >= n) return 0;
    return ((main + 31) >> 5) + ((n - main + 31) >> 5) == ((n + 31) >> 5) ? main : 0;
}

// Bounding circle of the points (S * px[i], S * py[i]) in the slots base .. base + 31 of the set (mm_tile_slot_point: the
// padding rows and columns of a tile duplicate a point, as the screen's fragments do).  Centre: middle of the bounding box.
// Radius: rounded UP -- the computed distance of a point from the centre carries at most 5 roundings of relative size 2^-24
// (difference, square, fma, sqrt), the factor 1 + 2^-18 covers 64 of them and 2^-10 covers the f32 underflow of squares of
// differences below 2^-60 -- so every point of the tile lies inside the circle, exactly.
MM_TB_HD inline void mm_tile_circle(const float* px, const float* py, int base, int n, float S, float* cx, float* cy, float* r,
                                    int main = 0)
{
    float x0 = INFINITY, x1 = -INFINITY, y0 = INFINITY, y1 = -INFINITY;
    for (int k = 0; k < 32; ++k) {
        const int i = mm_tile_slot_point(base + k, n, main);
        const float x = S * px[i], y = S * py[i];
        x0 = fminf(x0, x); x1 = fmaxf(x1, x); y0 = fminf(y0, y); y1 = fmaxf(y1, y);
    }
    const float mx = 0.5f * (x0 + x1), my = 0.5f * (y0 + y1);
    float m = 0.0f;
    for (int k = 0; k < 32; ++k) {
        const int i = mm_tile_slot_point(base + k, n, main);
        const float dx = S * px[i] - mx, dy = S * py[i] - my;
        m = fmaxf(m, fmaf(dx, dx, dy * dy));
    }
    *cx = mx; *cy = my;
    *r = mm_tb_sqrt(m) * 1.000003814697265625f + 0.0009765625f;       // (1 + 2^-18), 2^-10
}

// One circle for a column tile under EVERY rotation of a group: (ux, uy, r) is the tile's unrotated circle, cs the group's
// n >= 1 rotations as (cos, sin) pairs of f32, the values the columns are rotated by.  Centre: the tile's centre rotated
// (in f32, the fused form the kernel rotates by) by the middle rotation, cs[n / 2].  Radius: r plus the largest distance from
// there to the centre under any rotation of the group, that distance rounded UP as mm_tile_circle rounds a radius (its at
// most 5 relative roundings below the factor 1 + 2^-18; 2^-10 covers the underflow of the squares and the two additions
// here, 2^-13 each at magnitudes below 2^12).  A point of the tile under rotation g lies within r + 2^-11 of the centre
// rotated by g (mm_tile_gap), so within the returned radius + 2^-11 of the returned centre: mm_tile_gap of this circle is
// a lower bound for every rotation of the group.  Nothing is assumed of the rotations (far apart, unordered, repeated: the
// circle only grows; its radius stays below 2^12, which mm_tile_gap's slack covers).  n == 1: the circle mm_tile_gap
// takes today, bit for bit.
MM_TB_HD inline void mm_tile_group_circle(float ux, float uy, float r, const float* cs, int n, float* cx, float* cy, float* rg)
{
    const float cm = cs[2 * (n >> 1)], sm = cs[2 * (n >> 1) + 1];
    const float mx = fmaf(ux, cm, -(uy * sm)), my = fmaf(ux, sm, uy * cm);
    float m = 0.0f;
    for (int g = 0; g < n; ++g) {
        const float c = cs[2 * g], s = cs[2 * g + 1];
        const float dx = fmaf(ux, c, -(uy * s)) - mx, dy = fmaf(ux, s, uy * c) - my;
        m = fmaxf(m, fmaf(dx, dx, dy * dy));
    }
    *cx = mx; *cy = my;
    *rg = n > 1 ? r + (mm_tb_sqrt(m) * 1.000003814697265625f + 0.0009765625f) : r;   // (1 + 2^-18), 2^-10
}

// The group size the engine takes for a candidate list (radians), ScreenOptions::screen_group == 0: the largest G of 8, 4,
// 2 whose span (G - 1) * step is at most 3.5 degrees, step the median of the absolute differences of neighbours; else 1.
// A tile is an arc of some 22 degrees: a group that spans a sixth of it widens the circles by little.  The median ignores
// a jump (two concatenated ranges) and needs no order; a wrong guess costs tiles, never a value (mm_tile_group_circle).
inline int mm_tile_group_auto(const double* angles, int n)
{
    if (n < 2) return 1;
    std::vector<double> d((size_t)n - 1);
    for (int i = 0; i + 1 < n; ++i) d[(size_t)i] = std::fabs(angles[i + 1] - angles[i]);
    std::nth_element(d.begin(), d.begin() + (n - 1) / 2, d.end());
    const double step = d[(size_t)(n - 1) / 2] * 57.29577951308232;
    if (!(step == step)) return 1;
    for (int G = 8; G >= 2; G >>= 1)
        if ((G - 1) * step <= 3.5 * (1.0 + 1e-9)) return G;       // (a list of 0.5-degree steps in radians: 3.5 to rounding)
    return 1;
}

// Lower bound of the distance between a point of circle (ax, ay, ar) and a point of circle (bx, by, br), the second circle's
// centre rotated in f32 like its points (the rotation's roundings of a point and of the centre, and of the f32 cos / sin
// against the exact angle, move a point at most 2^-11 against its circle): |a - b| >= |ca - cb| - ar - br - 2^-11.  The
// computed |ca - cb| is at most 5 roundings (2^-24 each) above the exact one: the factor 1 - 2^-18 takes it below; the
// three subtractions round by at most 2^-13 each (magnitudes below 2^11); the slack 2^-7 holds both.  <= 0: no bound.
MM_TB_HD inline float mm_tile_gap(float ax, float ay, float ar, float bx, float by, float br)
{
    const float dx = ax - bx, dy = ay - by;
    const float d = mm_tb_sqrt(fmaf(dx, dx, dy * dy));
    return d * 0.999996185302734375f - (ar + br) - 0.0078125f;       // (1 - 2^-18), 2^-7
}

// Threshold of a tile pair: every SCREENED squared distance of the tile is >= the returned value (when it is > 0).
// gap <= the exact distance of any pair, so gap^2 <= the exact squared distance; the screen's value lies within e2s of the
// exact one (e2s = PairDesc::e2 in scaled units, rounded up).  gap^2 rounds once, the product with 1 - 2^-17 once, the
// difference once (relative to the product): (1 - 2^-17)(1 + 2^-24)^2 < 1 - 2^-24 keeps the result below gap^2 - e2s.
// Negative: no threshold (the circles are too close for any skip).
MM_TB_HD inline float mm_tile_threshold(float gap, float e2s)
{
    if (!(gap > 0.0f)) return -1.0f;
    const float g2 = gap * gap;
    return g2 * 0.99999237060546875f - e2s;                          // (1 - 2^-17)
}

// e2 (unscaled, f64) in scaled units, rounded up: 2^(2e) is exact, the conversion to f32 rounds by at most 2^-24
MM_TB_HD inline float mm_tile_e2s(double e2, int e)
{
    return (float)std::ldexp(e2, 2 * e) * 1.000003814697265625f;
}
