// mm_clip_device.h -- the per-face step of "mesh clipping" (include/mm_ccta.h, rule C4) as C++ for host and device: the
// rotation of a cut face to its apex, its three pieces, the shorter-diagonal rule of the quad, which pieces stay and
// which are null, and C2's per-face orphan test.  Every operation is unfused f64 in the order written (the files that include it are built with
// -ffp-contract=off), so the kernel (mm_clip_kernels.hip), the host hook (mm_clip.cpp), the stand-alone program
// (tests/clip_device_host.cpp) and the checker (tests/mm_checkers/mesh_clip.py) produce the same bits.  Selects only, no
// indexed arrays: on the device everything stays in registers.  Internal.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MM_CLIP_HD __host__ __device__ __forceinline__
#else
#define MM_CLIP_HD inline
#endif

namespace mm {
namespace clip {

// one record per cut face, 48 bytes, written by the host (mm_clip.cpp).  New vertices are named by their position among
// the new vertices of the call; the result's index is the number of kept old vertices plus that.
struct Record {
    int32_t face;          // the cut face
    int32_t flags;         // apex corner (bits 0-1) | the apex is on the kept side (bit 2) | LOOP cut (bit 3) | its rim edge
                           // lies on a closed loop (bit 4)
    int32_t cut;
    int32_t m_ab, m_ca;    // the loop points on the edges (a, b) and (c, a)
    int32_t r_ab, r_ca;    // their places in ring 1 of the cut (ring j: + (j - 1) * ring_stride); -1 on an open contour
    int32_t ring_stride;   // the points of the cut's closed loops
    int32_t centre;        // the centre of its loop among the new vertices, -1 without a cap
    int32_t ext_at;        // its first extension face, counted from the first extension face of the call (layer j: + j *
                           // 2 * ring_stride)
    int32_t cap_at;        // its cap face, counted from the first cap face of the call
    int32_t pad;
};
static_assert(sizeof(Record) == 48, "a clip record is 48 bytes");

constexpr int kApexMask = 3, kApexKept = 4, kLoopCut = 8, kClosedRim = 16;

struct Point { double x, y, z; };

// a corner of a piece: its name in the result (any int32 for a dropped vertex), its point, whether it is dropped
struct Corner { int32_t id; Point p; bool dropped; };

MM_CLIP_HD Corner pick(bool first, const Corner& a, const Corner& b)
{
    return Corner{first ? a.id : b.id, Point{first ? a.p.x : b.p.x, first ? a.p.y : b.p.y, first ? a.p.z : b.p.z},
                  first ? a.dropped : b.dropped};
}

MM_CLIP_HD double sq_dist(const Point& p, const Point& q)
{
    const double dx = p.x - q.x, dy = p.y - q.y, dz = p.z - q.z;
    return (dx * dx + dy * dy) + dz * dz;
}

MM_CLIP_HD bool same_point(const Point& p, const Point& q) { return p.x == q.x && p.y == q.y && p.z == q.z; }

struct Piece {
    int32_t i0, i1, i2;
    bool kept;             // none of its old vertices is dropped
    bool null;             // two corners of equal coordinates
};
struct Pieces { Piece apex, first, second; };

MM_CLIP_HD Piece piece(const Corner& p, const Corner& q, const Corner& r)
{
    return Piece{p.id, q.id, r.id, !(p.dropped || q.dropped || r.dropped),
                 same_point(p.p, q.p) || same_point(q.p, r.p) || same_point(p.p, r.p)};
}

// C4: the face (c0, c1, c2) rotated, winding preserved, to (a, b, c) with a = corner `apex`; m_ab and m_ca its loop
// points (never dropped).  The apex piece, then the quad m_ab, b, c, m_ca cut by its shorter diagonal, ties to b - m_ca.
MM_CLIP_HD Pieces face_pieces(const Corner& c0, const Corner& c1, const Corner& c2, int apex, const Corner& m_ab, const Corner& m_ca)
{
    const bool k0 = apex == 0, k1 = apex == 1;
    const Corner a = pick(k0, c0, pick(k1, c1, c2)), b = pick(k0, c1, pick(k1, c2, c0)), c = pick(k0, c2, pick(k1, c0, c1));
    const bool through_c = sq_dist(m_ab.p, c.p) < sq_dist(b.p, m_ca.p);
    Pieces out;
    out.apex = piece(a, m_ab, m_ca);
    out.first = piece(m_ab, b, pick(through_c, c, m_ca));
    out.second = piece(pick(through_c, m_ab, b), c, m_ca);
    return out;
}

// C2's orphan check for one cut face: its kept-side old vertices (the apex where the apex is kept, otherwise b and c)
// include a dropped one.  d0, d1, d2: whether the corners c0, c1, c2 of the face are dropped.
MM_CLIP_HD bool kept_side_dropped(int32_t flags, bool d0, bool d1, bool d2)
{
    const int apex = flags & kApexMask;
    const bool a = apex == 0 ? d0 : (apex == 1 ? d1 : d2);
    const bool others = apex == 0 ? (d1 || d2) : (apex == 1 ? (d2 || d0) : (d0 || d1));
    return (flags & kApexKept) ? a : others;
}

// C6: the kept side of a cut face runs x -> y along its rim edge: the apex piece runs m_ab -> m_ca, the quad's the other way
MM_CLIP_HD bool rim_runs_ab_to_ca(int32_t flags) { return (flags & kApexKept) != 0; }

}  // namespace clip
}  // namespace mm
