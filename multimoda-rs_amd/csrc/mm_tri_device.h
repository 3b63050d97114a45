// mm_tri_device.h -- the closest point of a triangle and its squared distance, as include/mm_ccta.h ("surface distance")
// states them: what k_tri_min / k_tri_closest (mm_tri_kernels.hip) fold over and what the mesh relaxation
// (mm_relax_kernels.hip) seeds its minima with -- one inlined face_d2, so a seed is a member of the set the fold
// runs over, bit for bit.  Every operation unfused and in the header's order (the files are built with
// -ffp-contract=off), every quotient a true division.  The vector helpers (V3, sub3, dot3, cross3, load3, len_sq3,
// tri_quality) also serve the flips and the collapse (mm_flip_kernels.hip, mm_collapse_kernels.hip).  Device code only.
#pragma once

#include <hip/hip_runtime.h>

namespace mm {

struct V3 { double x, y, z; };

__device__ __forceinline__ V3 sub3(const V3& u, const V3& v) { return V3{u.x - v.x, u.y - v.y, u.z - v.z}; }
__device__ __forceinline__ double dot3(const V3& u, const V3& v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }
// u + e * t, one rounding for each product and each sum
__device__ __forceinline__ V3 along(const V3& u, const V3& e, double t) { return V3{u.x + e.x * t, u.y + e.y * t, u.z + e.z * t}; }
__device__ __forceinline__ double dist2(const V3& p, const V3& q) { const V3 d = sub3(p, q); return dot3(d, d); }
// (u x w) with the component expressions of the degenerate test
__device__ __forceinline__ V3 cross3(const V3& u, const V3& w)
{
    return V3{u.y * w.z - u.z * w.y, u.z * w.x - u.x * w.z, u.x * w.y - u.y * w.x};
}
// point i of an array of xyz triples
__device__ __forceinline__ V3 load3(const double* p, long long i) { return V3{p[3 * i], p[3 * i + 1], p[3 * i + 2]}; }
// ((dx dx + dy dy) + dz dz) of d = q - p: the squared length of "mesh refinement"
__device__ __forceinline__ double len_sq3(const V3& p, const V3& q) { return dist2(q, p); }
// dot(n, n) / (S S) of the triangle (i, j, k) with normal n, S the sum of its squared edge lengths; 0 where S is 0
__device__ __forceinline__ double tri_quality(const V3& i, const V3& j, const V3& k, const V3& n)
{
    const double s = (len_sq3(i, j) + len_sq3(j, k)) + len_sq3(k, i);
    return s == 0.0 ? 0.0 : dot3(n, n) / (s * s);
}

// closest point of a proper face; ab = b - a, ac = c - a
__device__ __forceinline__ V3 tri_closest(const V3& p, const V3& a, const V3& b, const V3& c, const V3& ab, const V3& ac,
                                          int& region)
{
    const V3 ap = sub3(p, a);
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) { region = 1; return a; }
    const V3 bp = sub3(p, b);
    const double d3 = dot3(ab, bp), d4 = dot3(ac, bp);
    if (d3 >= 0.0 && d4 <= d3) { region = 2; return b; }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) { region = 4; return along(a, ab, d1 / (d1 - d3)); }
    const V3 cp = sub3(p, c);
    const double d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) { region = 3; return c; }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) { region = 6; return along(a, ac, d2 / (d2 - d6)); }
    const double va = d3 * d6 - d5 * d4;
    const double e43 = d4 - d3, e56 = d5 - d6;
    if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) { region = 5; return along(b, sub3(c, b), e43 / (e43 + e56)); }
    const double s = (va + vb) + vc;
    region = 0;
    return along(along(a, ab, vb / s), ac, vc / s);
}

// closest point of the segment (u, v)
__device__ __forceinline__ V3 seg_closest(const V3& p, const V3& u, const V3& v)
{
    const V3 e = sub3(v, u);
    const double l = dot3(e, e);
    double t = 0.0;
    if (l != 0.0) {
        t = dot3(sub3(p, u), e) / l;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);   // a NaN stays a NaN
    }
    return along(u, e, t);
}

// the nearest of ab, bc, ca, the first on ties; best = its squared distance
__device__ __forceinline__ V3 segments_closest(const V3& p, const V3& a, const V3& b, const V3& c, int& region, double& best)
{
    V3 q = seg_closest(p, a, b);
    best = dist2(p, q);
    region = 4;
    const V3 q2 = seg_closest(p, b, c);
    const double v2 = dist2(p, q2);
    if (v2 < best) { best = v2; q = q2; region = 5; }
    const V3 q3 = seg_closest(p, c, a);
    const double v3 = dist2(p, q3);
    if (v3 < best) { best = v3; q = q3; region = 6; }
    return q;
}

// closest point of a degenerate face: its segments
__device__ __forceinline__ V3 degenerate_closest(const V3& p, const V3& a, const V3& b, const V3& c, int& region)
{
    double best;
    return segments_closest(p, a, b, c, region, best);
}

// closest point of a thin face: its segments, then the interior point where all three of va, vb, vc are positive (the
// point is then a convex combination of the corners) and it is strictly nearer
__device__ __forceinline__ V3 thin_closest(const V3& p, const V3& a, const V3& b, const V3& c, const V3& ab, const V3& ac,
                                           int& region)
{
    double best;
    V3 q = segments_closest(p, a, b, c, region, best);
    const V3 ap = sub3(p, a), bp = sub3(p, b), cp = sub3(p, c);
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap);
    const double d3 = dot3(ab, bp), d4 = dot3(ac, bp);
    const double d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    const double vc = d1 * d4 - d3 * d2;
    const double vb = d5 * d2 - d1 * d6;
    const double va = d3 * d6 - d5 * d4;
    if (va > 0.0 && vb > 0.0 && vc > 0.0) {
        const double s = (va + vb) + vc;
        const V3 q0 = along(along(a, ab, vb / s), ac, vc / s);
        if (dist2(p, q0) < best) { q = q0; region = 0; }
    }
    return q;
}

// the kind of a staged face, as the bits of a.w carry it (mm_tri_plan.h: face_kind)
enum : int { kFaceProper = 0, kFaceDegenerate = 1, kFaceThin = 2 };

__device__ __forceinline__ V3 face_closest(const V3& p, const V3& a, const V3& b, const V3& c, const V3& ab, const V3& ac,
                                           int kind, int& region)
{
    if (kind == kFaceProper) return tri_closest(p, a, b, c, ab, ac, region);
    if (kind == kFaceDegenerate) return degenerate_closest(p, a, b, c, region);
    return thin_closest(p, a, b, c, ab, ac, region);
}

__device__ __forceinline__ double face_d2(const V3& p, const V3& a, const V3& b, const V3& c, const V3& ab, const V3& ac,
                                          int kind)
{
    int region;
    return dist2(p, face_closest(p, a, b, c, ab, ac, kind, region));
}

}  // namespace mm
