// mm_section_device.h -- the arithmetic of "mesh cross-sections" (include/mm_ccta.h), rules 1 to 4 and 8, as C++ for
// host and device: the height of a point over a plane, its side, the crossing point of an edge, the segment a crossed
// face gives, and the extreme heights of a box.  Every operation is unfused f64 in the order written (the files that
// include it are built with -ffp-contract=off), so the kernel (mm_section_kernels.hip), the host plan and the host test
// hook (mm_section.cpp) and the checker (tests/mm_checkers/mesh_sections.py) produce the same bits.  Internal.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MM_SECTION_HD __host__ __device__ __forceinline__
#else
#define MM_SECTION_HD inline
#endif

namespace mm {
namespace section {

constexpr int kChunk = 256;      // faces a chunk, one per lane
constexpr int kPlaneRun = 64;    // planes a work item: 64 x 48 bytes of LDS

// origin xyz, normal xyz: 48 bytes
struct Plane { double ox, oy, oz, nx, ny, nz; };

// one record per (plane, crossed face), 72 bytes: key = plane << 32 | original face index; e = the two edge keys
// (lo, hi by vertex index), the smaller key first; p = their points in that order
struct Segment {
    unsigned long long key;
    int32_t e[4];
    double p[6];
};
static_assert(sizeof(Segment) == 72, "a segment record is 72 bytes");

// rule 1
MM_SECTION_HD double height(const Plane& pl, double x, double y, double z)
{
    return (pl.nx * (x - pl.ox) + pl.ny * (y - pl.oy)) + pl.nz * (z - pl.oz);
}
MM_SECTION_HD int side(double h) { return h < 0.0 ? 0 : 1; }

// a corner of a face: coordinates, height over the plane, vertex index
struct Corner { double x, y, z, h; int32_t id; };
struct EdgePoint { int32_t lo, hi; double x, y, z; };

MM_SECTION_HD Corner pick(bool first, const Corner& a, const Corner& b)
{
    return Corner{first ? a.x : b.x, first ? a.y : b.y, first ? a.z : b.z, first ? a.h : b.h, first ? a.id : b.id};
}

// rule 3: the point of the crossed edge (a, b), always from the lower index to the higher
MM_SECTION_HD EdgePoint crossing(const Corner& a, const Corner& b)
{
    const bool a_lo = a.id < b.id;
    const Corner lo = pick(a_lo, a, b), hi = pick(a_lo, b, a);
    const double t = lo.h / (lo.h - hi.h);
    return EdgePoint{lo.id, hi.id, lo.x + t * (hi.x - lo.x), lo.y + t * (hi.y - lo.y), lo.z + t * (hi.z - lo.z)};
}

// rule 2 for one face of three distinct indices: do its corners' heights lie on both sides
MM_SECTION_HD bool crossed(double h0, double h1, double h2)
{
    const int s0 = side(h0), s1 = side(h1), s2 = side(h2);
    return !(s0 == s1 && s1 == s2);
}

// rules 3 and 4 for a crossed face.  Selects only, no indexed arrays: on the device everything stays in registers.
MM_SECTION_HD void cut_face(const Corner& c0, const Corner& c1, const Corner& c2, unsigned long long key, Segment& s)
{
    const int s0 = side(c0.h), s1 = side(c1.h), s2 = side(c2.h);
    // the corner alone on its side comes first: its two edges are the crossed ones
    const bool k2 = s0 == s1, k1 = !k2 && s0 == s2;
    const Corner a = pick(k2, c2, pick(k1, c1, c0)), b = pick(k2, c0, pick(k1, c2, c1)), c = pick(k2, c1, pick(k1, c0, c2));
    const EdgePoint u = crossing(a, b), w = crossing(a, c);
    const bool swap = w.lo < u.lo || (w.lo == u.lo && w.hi < u.hi);
    s.key = key;
    s.e[0] = swap ? w.lo : u.lo; s.e[1] = swap ? w.hi : u.hi; s.e[2] = swap ? u.lo : w.lo; s.e[3] = swap ? u.hi : w.hi;
    s.p[0] = swap ? w.x : u.x; s.p[1] = swap ? w.y : u.y; s.p[2] = swap ? w.z : u.z;
    s.p[3] = swap ? u.x : w.x; s.p[4] = swap ? u.y : w.y; s.p[5] = swap ? u.z : w.z;
}

// rule 8: the least and the greatest height over the box lo .. hi, taken at the corners the signs of n pick
MM_SECTION_HD void box_heights(const Plane& pl, const double* lo, const double* hi, double& h_min, double& h_max)
{
    const bool px = !(pl.nx < 0.0), py = !(pl.ny < 0.0), pz = !(pl.nz < 0.0);
    h_min = height(pl, px ? lo[0] : hi[0], py ? lo[1] : hi[1], pz ? lo[2] : hi[2]);
    h_max = height(pl, px ? hi[0] : lo[0], py ? hi[1] : lo[1], pz ? hi[2] : lo[2]);
}
MM_SECTION_HD bool box_takes_part(double h_min, double h_max) { return h_min < 0.0 && !(h_max < 0.0); }

}  // namespace section
}  // namespace mm
