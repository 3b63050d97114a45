// mm_isect_device.h -- the narrow phase of the mesh intersection check (include/mm_ccta.h, "mesh intersections"): the
// filtered orientation predicates and the state of one pair of proper faces.  Every function is MM_HD and plain C++: the
// device runs it (mm_intersect_kernels.hip) and a host compiler builds the same text; tests/mm_checkers/
// mesh_intersections.py restates it line by line.  All arithmetic is unfused f64 in the order written (the build passes
// -ffp-contract=off).  Corners are permuted by selects on their components, never by a runtime index or a conditional
// between whole points: either would put the points into scratch memory.
#pragma once

#include "mm_prune.h"   // MM_HD

namespace mm {
namespace isect {

enum : int { kDisjoint = 0, kIntersecting = 1, kUndecided = 2, kCoincident = 4 };   // kCoincident rides on kIntersecting

struct P3 { double x, y, z; };
struct P2 { double u, v; };

// stage A of the published adaptive predicates (Shewchuk 1997), epsilon = 2^-53
constexpr double kEps = 1.1102230246251565e-16;
constexpr double kO3dBound = (7.0 + 56.0 * kEps) * kEps;
constexpr double kO2dBound = (3.0 + 16.0 * kEps) * kEps;
constexpr double kTiny = 0x1p-900;                   // 2^-900, as a power of two and not in decimal digits
constexpr double kHuge = 1.7976931348623157e308;     // DBL_MAX: `perm <= kHuge` is false for +inf and NaN

MM_HD inline double absd(double x) { return __builtin_fabs(x); }

// The sign of det[a - d; b - d; c - d] where the bound proves it, else 0.
MM_HD inline int orient3d(const P3& a, const P3& b, const P3& c, const P3& d)
{
    const double adx = a.x - d.x, bdx = b.x - d.x, cdx = c.x - d.x;
    const double ady = a.y - d.y, bdy = b.y - d.y, cdy = c.y - d.y;
    const double adz = a.z - d.z, bdz = b.z - d.z, cdz = c.z - d.z;
    const double bdxcdy = bdx * cdy, cdxbdy = cdx * bdy;
    const double cdxady = cdx * ady, adxcdy = adx * cdy;
    const double adxbdy = adx * bdy, bdxady = bdx * ady;
    const double det = (adz * (bdxcdy - cdxbdy) + bdz * (cdxady - adxcdy)) + cdz * (adxbdy - bdxady);
    const double perm = ((absd(bdxcdy) + absd(cdxbdy)) * absd(adz) + (absd(cdxady) + absd(adxcdy)) * absd(bdz))
                        + (absd(adxbdy) + absd(bdxady)) * absd(cdz);
    if (!(perm <= kHuge) || perm < kTiny) return 0;
    const double bound = kO3dBound * perm;
    return det > bound ? 1 : (-det > bound ? -1 : 0);
}

// The sign of det[a - c; b - c] where the bound proves it, else 0.
MM_HD inline int orient2d(const P2& a, const P2& b, const P2& c)
{
    const double left = (a.u - c.u) * (b.v - c.v);
    const double right = (a.v - c.v) * (b.u - c.u);
    const double det = left - right;
    const double detsum = absd(left) + absd(right);
    if (!(detsum <= kHuge) || detsum < kTiny) return 0;
    const double bound = kO2dBound * detsum;
    return det > bound ? 1 : (-det > bound ? -1 : 0);
}

// the axis of the largest |component| of (q - p) x (r - p), the first of equal ones
MM_HD inline int dominant_axis(const P3& p, const P3& q, const P3& r)
{
    const double ux = q.x - p.x, uy = q.y - p.y, uz = q.z - p.z;
    const double vx = r.x - p.x, vy = r.y - p.y, vz = r.z - p.z;
    const double nx = absd(uy * vz - uz * vy), ny = absd(uz * vx - ux * vz), nz = absd(ux * vy - uy * vx);
    int ax = 0;
    double m = nx;
    if (ny > m) { ax = 1; m = ny; }
    if (nz > m) ax = 2;
    return ax;
}

MM_HD inline P2 drop(const P3& p, int ax) { return P2{ax == 0 ? p.y : p.x, ax == 2 ? p.y : p.z}; }

// Selections go component by component: a conditional between whole points selects an address, and the points would
// have to live in memory.
MM_HD inline P3 pick(bool c, const P3& a, const P3& b) { return P3{c ? a.x : b.x, c ? a.y : b.y, c ? a.z : b.z}; }
MM_HD inline P3 pick3(int k, const P3& a, const P3& b, const P3& c) { return pick(k == 0, a, pick(k == 1, b, c)); }

MM_HD inline void swap_if(bool c, P3& a, P3& b) { const P3 t = pick(c, b, a); b = pick(c, a, b); a = t; }

// (p, q, r) -> the rotation that starts at corner k
MM_HD inline void rotate_to(P3& p, P3& q, P3& r, int k)
{
    const P3 a = pick3(k, p, q, r), b = pick3(k, q, r, p), c = pick3(k, r, p, q);
    p = a; q = b; r = c;
}

// an edge of the 2-D triangle (a, b, c) with u0, u1, u2 certainly on its outer side
MM_HD inline bool edge_separates(const P2& a, const P2& b, const P2& c, const P2& u0, const P2& u1, const P2& u2)
{
    const int inner = orient2d(a, b, c);
    if (inner == 0) return false;
    return orient2d(a, b, u0) == -inner && orient2d(a, b, u1) == -inner && orient2d(a, b, u2) == -inner;
}

MM_HD inline bool separated_2d(const P2& a, const P2& b, const P2& c, const P2& u0, const P2& u1, const P2& u2)
{
    return edge_separates(a, b, c, u0, u1, u2) || edge_separates(b, c, a, u0, u1, u2) || edge_separates(c, a, b, u0, u1, u2);
}

// the edge a b of the 2-D triangle (a, b, c), one end of it a vertex shared with the other triangle, whose two other
// corners u1, u2 are certainly on its outer side
MM_HD inline bool wedge_separates(const P2& a, const P2& b, const P2& c, const P2& u1, const P2& u2)
{
    const int inner = orient2d(a, b, c);
    return inner != 0 && orient2d(a, b, u1) == -inner && orient2d(a, b, u2) == -inner;
}

// three certain signs, not all equal: the one that differs from the other two
MM_HD inline int lone(int s0, int s1, int s2) { return s1 == s2 ? 0 : (s0 == s2 ? 1 : 2); }

MM_HD inline int no_shared(P3 p1, P3 q1, P3 r1, P3 p2, P3 q2, P3 r2)
{
    const int a0 = orient3d(p1, q1, r1, p2), a1 = orient3d(p1, q1, r1, q2), a2 = orient3d(p1, q1, r1, r2);
    if (a0 != 0 && a0 == a1 && a0 == a2) return kDisjoint;
    const int b0 = orient3d(p2, q2, r2, p1), b1 = orient3d(p2, q2, r2, q1), b2 = orient3d(p2, q2, r2, r1);
    if (b0 != 0 && b0 == b1 && b0 == b2) return kDisjoint;
    if ((a0 | a1 | a2 | b0 | b1 | b2) == 0) {                         // nearly coplanar
        const int ax = dominant_axis(p1, q1, r1);
        const P2 s0 = drop(p1, ax), s1 = drop(q1, ax), s2 = drop(r1, ax);
        const P2 t0 = drop(p2, ax), t1 = drop(q2, ax), t2 = drop(r2, ax);
        return separated_2d(s0, s1, s2, t0, t1, t2) || separated_2d(t0, t1, t2, s0, s1, s2) ? kDisjoint : kUndecided;
    }
    if (a0 == 0 || a1 == 0 || a2 == 0 || b0 == 0 || b1 == 0 || b2 == 0) return kUndecided;
    // b: the corners of face 1 against the plane of face 2; a: those of face 2 against the plane of face 1
    const int k1 = lone(b0, b1, b2), k2 = lone(a0, a1, a2);
    const int lone1 = k1 == 0 ? b0 : (k1 == 1 ? b1 : b2), lone2 = k2 == 0 ? a0 : (k2 == 1 ? a1 : a2);
    rotate_to(p1, q1, r1, k1);
    rotate_to(p2, q2, r2, k2);
    swap_if(lone1 < 0, q2, r2);
    swap_if(lone2 < 0, q1, r1);
    const int e1 = orient3d(p1, q1, p2, q2);
    if (e1 > 0) return kDisjoint;
    const int e2 = orient3d(p1, r1, r2, p2);
    if (e2 > 0) return kDisjoint;
    return e1 < 0 && e2 < 0 ? kIntersecting : kUndecided;
}

// the segment q r (plane signs sq, sr against the triangle) and the triangle (t0, t1, t2)
MM_HD inline void edge_against(const P3& q, const P3& r, int sq, int sr, const P3& t0, const P3& t1, const P3& t2,
                               bool& crossing, bool& missing)
{
    const int e0 = orient3d(q, r, t0, t1), e1 = orient3d(q, r, t1, t2), e2 = orient3d(q, r, t2, t0);
    crossing = sq != 0 && sr == -sq && e0 != 0 && e0 == e1 && e0 == e2;
    missing = (e0 > 0 || e1 > 0 || e2 > 0) && (e0 < 0 || e1 < 0 || e2 < 0);
}

// k1, k2: the shared corner in each face
MM_HD inline int one_shared(P3 p1, P3 q1, P3 r1, int k1, P3 p2, P3 q2, P3 r2, int k2)
{
    rotate_to(p1, q1, r1, k1);
    rotate_to(p2, q2, r2, k2);
    const int a1 = orient3d(p2, q2, r2, q1), b1 = orient3d(p2, q2, r2, r1);
    if (a1 != 0 && a1 == b1) return kDisjoint;
    const int a2 = orient3d(p1, q1, r1, q2), b2 = orient3d(p1, q1, r1, r2);
    if (a2 != 0 && a2 == b2) return kDisjoint;
    bool cross1, miss1, cross2, miss2;
    edge_against(q1, r1, a1, b1, p2, q2, r2, cross1, miss1);
    if (cross1) return kIntersecting;
    edge_against(q2, r2, a2, b2, p1, q1, r1, cross2, miss2);
    if (cross2) return kIntersecting;
    if (miss1 && miss2) return kDisjoint;
    if ((a1 | b1 | a2 | b2) != 0) return kUndecided;
    // nearly coplanar: the two edges of each face at the shared vertex, in the dominant projection of face 1
    const int ax = dominant_axis(p1, q1, r1);
    const P2 s0 = drop(p1, ax), s1 = drop(q1, ax), s2 = drop(r1, ax);
    const P2 t0 = drop(p2, ax), t1 = drop(q2, ax), t2 = drop(r2, ax);
    return wedge_separates(s0, s1, s2, t1, t2) || wedge_separates(s2, s0, s1, t1, t2) ||
           wedge_separates(t0, t1, t2, s1, s2) || wedge_separates(t2, t0, t1, s1, s2) ? kDisjoint : kUndecided;
}

// k1, k2: the corner of each face that the other does not have
MM_HD inline int two_shared(const P3& p1, const P3& q1, const P3& r1, int k1, const P3& p2, const P3& q2, const P3& r2, int k2)
{
    P3 c1 = p1, a = q1, b = r1;
    rotate_to(c1, a, b, k1);
    const P3 c2 = pick3(k2, p2, q2, r2);
    if (orient3d(p1, q1, r1, c2) != 0 || orient3d(p2, q2, r2, c1) != 0) return kDisjoint;
    const int ax = dominant_axis(p1, q1, r1);
    const P2 a2 = drop(a, ax), b2 = drop(b, ax);
    const int s1 = orient2d(a2, b2, drop(c1, ax)), s2 = orient2d(a2, b2, drop(c2, ax));
    return s1 != 0 && s2 == -s1 ? kDisjoint : kUndecided;
}

// The state of two proper faces; i*: the canonical vertex ids of their corners (distinct within a face).  In the self
// form face 1 is the one with the lower index.  kIntersecting | kCoincident for three shared vertices.
MM_HD inline int pair_state(const P3& p1, const P3& q1, const P3& r1, int ip1, int iq1, int ir1, const P3& p2, const P3& q2,
                            const P3& r2, int ip2, int iq2, int ir2)
{
    const bool in0 = ip1 == ip2 || ip1 == iq2 || ip1 == ir2;          // corner of face 1 found in face 2
    const bool in1 = iq1 == ip2 || iq1 == iq2 || iq1 == ir2;
    const bool in2 = ir1 == ip2 || ir1 == iq2 || ir1 == ir2;
    const int n = (int)in0 + (int)in1 + (int)in2;
    if (n == 0) return no_shared(p1, q1, r1, p2, q2, r2);
    const bool on0 = ip2 == ip1 || ip2 == iq1 || ip2 == ir1;          // corner of face 2 found in face 1
    const bool on1 = iq2 == ip1 || iq2 == iq1 || iq2 == ir1;
    if (n == 1) return one_shared(p1, q1, r1, in0 ? 0 : (in1 ? 1 : 2), p2, q2, r2, on0 ? 0 : (on1 ? 1 : 2));
    if (n == 2) return two_shared(p1, q1, r1, !in0 ? 0 : (!in1 ? 1 : 2), p2, q2, r2, !on0 ? 0 : (!on1 ? 1 : 2));
    return kIntersecting | kCoincident;
}

}  // namespace isect
}  // namespace mm
