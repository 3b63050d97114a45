// mm_clip.cpp -- mesh clipping (include/mm_ccta.h, "mesh clipping"): a mesh cut open along plane sections, one side of
// every cut thrown away by connectivity, the rims capped or extended.  Nothing in the reference does this.  The host
// checks the arguments, runs the section engine for the K planes (mm_mesh_sections; the hook runs its host form), reads
// the cut sets off the loops (C1: NO_LOOP, OVERLAP), and writes one record per cut face, the new vertices (loop points,
// rings, centres: C5, C6) and the rims.  Connectivity (C2), the pieces (C4) and the faces (C7) run on the device
// (mm_clip_kernels.hip) with the mesh resident from one upload to one download; mm_mesh_clip_host runs the same rule in
// host C++ with a sequential union-find and the per-face step of mm_clip_device.h.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <unordered_map>
#include <vector>

#include "../../include/mm_ccta.h"
#include "mm_clip_device.h"
#include "mm_section_device.h"
#include "mm_tri_plan.h"

using namespace mm;
using clip::Record;

static_assert(MM_CLIP_SCOPE_PLANE == kClipScopePlane && MM_CLIP_NOT_SEPARATING == kClipNotSeparating &&
              MM_CLIP_KEPT_SIDE_DROPPED == kClipKeptSideDropped, "the kernels' constants");
static_assert(MM_CLIP_KIND_UNTOUCHED == kClipUntouched && MM_CLIP_KIND_PIECE == kClipPiece &&
              MM_CLIP_KIND_EXTENSION == kClipExtension && MM_CLIP_KIND_CAP == kClipCap, "the kernels' face kinds");
static_assert(MM_CLIP_KEEP_BELOW == 0 && MM_CLIP_KEEP_ABOVE == 1, "keep is the side of rule 1 that stays");
static_assert(sizeof(mm_clip_report) == 144, "mm_clip_report is 144 bytes");

namespace {

struct Sections {
    std::vector<int64_t> contour_off, point_edge, point_face, contour_plane, plane_off, selected;
    std::vector<double> points, area, length, centroid;
    std::vector<int8_t> kind;
    void size(int64_t cap, int64_t K)
    {
        const size_t c = (size_t)std::max<int64_t>(cap, 1);
        contour_off.assign(c + 1, 0); points.assign(6 * c, 0.0); point_edge.assign(4 * c, 0); point_face.assign(2 * c, 0);
        contour_plane.assign(c, 0); kind.assign(c, 0); area.assign(c, 0.0); length.assign(c, 0.0); centroid.assign(3 * c, 0.0);
        plane_off.assign((size_t)K + 1, 0); selected.assign((size_t)std::max<int64_t>(K, 1), -1);
    }
};

struct Args {
    const double* v; int64_t nv; const int64_t* f; int64_t nf;
    const double *origins, *normals; const int32_t *keep, *scope; int64_t K;
    int cap; double ext_length; int64_t L;
};

// C1, C5, C6 on the host: everything but connectivity and pieces
struct Plan {
    std::vector<int64_t> info;         // per cut: status, loop points, closed loops, cut faces
    std::vector<double> measures;      // per cut: area, perimeter, centroid xyz
    std::vector<Record> rec;
    std::vector<double> newv;          // the new vertices, cut after cut
    std::vector<int32_t> new_cut;
    std::vector<int64_t> rim_off, rim; // per closed loop the outermost ring, as names among the new vertices
    int64_t n_ext = 0, n_cap = 0, n_closed = 0, n_open = 0;
    bool ok = true;                    // every status OK after C1
    int64_t n_new() const { return (int64_t)new_cut.size(); }
};

struct Out {
    int64_t vert_cap, face_cap;
    double* vertices; int64_t *tris, *vertex_origin, *face_origin; int8_t* face_kind;
    int64_t* cut_status; double* cut_measures; int64_t *rim_off, *rim_index;
    mm_clip_report* report;
};

int check_args(const Args& a, const Out& o, const char* who)
{
    if (!o.report || !o.rim_off || o.vert_cap < 0 || o.face_cap < 0 || a.K < 0 || a.K > kMaxIndex ||
        (a.K > 0 && (!a.origins || !a.normals || !a.keep || !a.scope || !o.cut_status || !o.cut_measures)) ||
        (o.vert_cap > 0 && (!o.vertices || !o.vertex_origin || !o.rim_index)) ||
        (o.face_cap > 0 && (!o.tris || !o.face_origin || !o.face_kind)))
        return set_error(MM_ERR_INVALID, std::string(who) + ": bad arguments");
    if (const int rc = plan_args(a.v, a.nv, a.f, a.nf, nullptr, 0, who)) return rc;
    for (int64_t k = 0; k < 3 * a.K; ++k)
        if (!std::isfinite(a.origins[k])) return set_error(MM_ERR_INVALID, std::string(who) + ": non-finite cut origin");
    for (int64_t k = 0; k < a.K; ++k) {
        const double* n = a.normals + 3 * k;
        if (!std::isfinite(n[0]) || !std::isfinite(n[1]) || !std::isfinite(n[2]))
            return set_error(MM_ERR_INVALID, std::string(who) + ": non-finite cut normal");
        if (n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0) return set_error(MM_ERR_INVALID, std::string(who) + ": zero cut normal");
        if (a.keep[k] != MM_CLIP_KEEP_BELOW && a.keep[k] != MM_CLIP_KEEP_ABOVE)
            return set_error(MM_ERR_INVALID, std::string(who) + ": keep must be MM_CLIP_KEEP_BELOW or MM_CLIP_KEEP_ABOVE");
        if (a.scope[k] != MM_CLIP_SCOPE_LOOP && a.scope[k] != MM_CLIP_SCOPE_PLANE)
            return set_error(MM_ERR_INVALID, std::string(who) + ": scope must be MM_CLIP_SCOPE_LOOP or MM_CLIP_SCOPE_PLANE");
    }
    if (a.cap != 0 && a.cap != 1) return set_error(MM_ERR_INVALID, std::string(who) + ": cap must be 0 or 1");
    if (!std::isfinite(a.ext_length) || a.ext_length < 0.0 || a.L < 0 || a.L > (1 << 20))
        return set_error(MM_ERR_INVALID, std::string(who) + ": ext_length must be finite and >= 0, ext_layers in [0, 2^20]");
    if ((a.ext_length == 0.0) != (a.L == 0))
        return set_error(MM_ERR_INVALID, std::string(who) + ": ext_length and ext_layers are zero together or not at all");
    return MM_OK;
}

section::Plane plane_of(const Args& a, int64_t k)
{
    return section::Plane{a.origins[3 * k], a.origins[3 * k + 1], a.origins[3 * k + 2], a.normals[3 * k], a.normals[3 * k + 1], a.normals[3 * k + 2]};
}

int vertex_side(const Args& a, const section::Plane& pl, int64_t i)
{
    return section::side(section::height(pl, a.v[3 * i], a.v[3 * i + 1], a.v[3 * i + 2]));
}

// the sections of the K planes without a device: the hooks of mm_section.cpp
int sections_on_host(const Args& a, Sections& s)
{
    int64_t n = 0, counts[5];
    int rc = mm_section_cut_host(a.v, a.nv, a.f, a.nf, a.origins, a.normals, a.K, 0, nullptr, &n);
    if (rc) return rc;
    std::vector<section::Segment> seg((size_t)std::max<int64_t>(n, 1));
    if ((rc = mm_section_cut_host(a.v, a.nv, a.f, a.nf, a.origins, a.normals, a.K, n, seg.data(), &n))) return rc;
    s.size(n, a.K);
    return mm_section_chain(n ? seg.data() : nullptr, n, a.origins, a.normals, a.K, s.contour_off.data(), s.points.data(), s.point_edge.data(),
                            s.point_face.data(), s.contour_plane.data(), s.kind.data(), s.area.data(), s.length.data(),
                            s.centroid.data(), s.plane_off.data(), s.selected.data(), counts);
}

int sections_on_device(mm_engine* h, const Args& a, Sections& s)
{
    mm_section_report rep;
    // a plane through a tube of nf faces crosses about sqrt(nf) of them; the second call covers everything else
    int64_t cap = std::min<int64_t>(std::min<int64_t>(a.nf * a.K, a.K * (int64_t)std::sqrt((double)a.nf) + 4096), kMaxIndex);
    for (int attempt = 0;; ++attempt) {
        s.size(cap, a.K);
        const int rc = mm_mesh_sections(h, a.v, a.nv, a.f, a.nf, a.origins, a.normals, a.K, cap, s.contour_off.data(), s.points.data(),
                                        s.point_edge.data(), s.point_face.data(), s.contour_plane.data(), s.kind.data(), s.area.data(),
                                        s.length.data(), s.centroid.data(), s.plane_off.data(), s.selected.data(), &rep);
        if (rc == MM_ERR_TOO_LARGE && attempt == 0 && rep.n_segments > cap) { cap = rep.n_segments; continue; }
        return rc;
    }
}

unsigned long long edge_of(int64_t p, int64_t q)
{
    return (unsigned long long)std::min(p, q) << 32 | (unsigned long long)std::max(p, q);
}

int build_plan(const Args& a, const Sections& s, const char* who, Plan& pl)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const int64_t K = a.K, L = a.L;
    pl.info.assign((size_t)(4 * K), 0);
    pl.measures.assign((size_t)(5 * K), nan);
    pl.rim_off.assign(1, 0);
    std::vector<int32_t> owner((size_t)a.nf, -1);
    std::vector<std::vector<int32_t>> faces((size_t)K);
    std::vector<int64_t> c_lo((size_t)K), c_hi((size_t)K);

    // ---- C1
    for (int64_t k = 0; k < K; ++k) {
        std::vector<int32_t>& mine = faces[(size_t)k];
        if (a.scope[k] == MM_CLIP_SCOPE_LOOP) {
            const int64_t c = s.selected[(size_t)k];
            const bool found = c >= 0 && s.contour_off[(size_t)c + 1] - s.contour_off[(size_t)c] >= 3;
            c_lo[(size_t)k] = found ? c : 0;
            c_hi[(size_t)k] = found ? c + 1 : 0;
            if (!found) pl.info[(size_t)(4 * k)] = MM_CLIP_NO_LOOP;
            else
                for (int64_t i = s.contour_off[(size_t)c]; i < s.contour_off[(size_t)c + 1]; ++i) mine.push_back((int32_t)s.point_face[(size_t)i]);
        } else {
            c_lo[(size_t)k] = s.plane_off[(size_t)k];
            c_hi[(size_t)k] = s.plane_off[(size_t)k + 1];
            if (c_hi[(size_t)k] > c_lo[(size_t)k]) {              // every crossed face, branched contours included: rules 1 and 2
                const section::Plane plane = plane_of(a, k);
                for (int64_t i = 0; i < a.nf; ++i) {
                    const int64_t* t = a.f + 3 * i;
                    if (t[0] == t[1] || t[1] == t[2] || t[0] == t[2]) continue;
                    const int s0 = vertex_side(a, plane, t[0]), s1 = vertex_side(a, plane, t[1]), s2 = vertex_side(a, plane, t[2]);
                    if (!(s0 == s1 && s1 == s2)) mine.push_back((int32_t)i);
                }
            }
        }
        for (int64_t c = c_lo[(size_t)k]; c < c_hi[(size_t)k]; ++c) {
            pl.info[(size_t)(4 * k + 1)] += s.contour_off[(size_t)c + 1] - s.contour_off[(size_t)c];
            if (s.kind[(size_t)c] != MM_SECTION_CLOSED) continue;
            if (pl.info[(size_t)(4 * k + 2)]++ == 0) {
                pl.measures[(size_t)(5 * k)] = s.area[(size_t)c];
                pl.measures[(size_t)(5 * k + 1)] = s.length[(size_t)c];
                std::memcpy(&pl.measures[(size_t)(5 * k + 2)], &s.centroid[(size_t)(3 * c)], 24);
            }
        }
        pl.info[(size_t)(4 * k + 3)] = (int64_t)mine.size();
        for (int32_t face : mine) {
            int32_t& o = owner[(size_t)face];
            if (o >= 0 && o != k) pl.info[(size_t)(4 * k)] = pl.info[(size_t)(4 * o)] = MM_CLIP_OVERLAP;
            if (o < 0) o = (int32_t)k;
        }
    }
    for (int64_t k = 0; k < K; ++k) pl.ok = pl.ok && pl.info[(size_t)(4 * k)] == MM_CLIP_OK;
    if (!pl.ok) return MM_OK;

    // ---- C5 and C6: the new vertices, cut after cut, and a record per cut face
    std::vector<int32_t> rec_of((size_t)a.nf, -1);
    std::unordered_map<unsigned long long, int32_t> name_of_edge;
    std::vector<int32_t> crank;                                    // per loop point of the cut: its place among the closed loops' points
    for (int64_t k = 0; k < K; ++k) {
        const section::Plane plane = plane_of(a, k);
        const int64_t base = pl.n_new();
        name_of_edge.clear();
        crank.clear();
        int64_t closed_points = 0;
        for (int64_t c = c_lo[(size_t)k]; c < c_hi[(size_t)k]; ++c)
            for (int64_t i = s.contour_off[(size_t)c]; i < s.contour_off[(size_t)c + 1]; ++i) {
                name_of_edge[edge_of(s.point_edge[(size_t)(2 * i)], s.point_edge[(size_t)(2 * i + 1)])] = (int32_t)pl.n_new();
                crank.push_back(s.kind[(size_t)c] == MM_SECTION_CLOSED ? (int32_t)closed_points++ : -1);
                pl.newv.insert(pl.newv.end(), &s.points[(size_t)(3 * i)], &s.points[(size_t)(3 * i)] + 3);
                pl.new_cut.push_back((int32_t)k);
            }
        const int64_t ring1 = pl.n_new();
        const double nn = std::sqrt((plane.nx * plane.nx + plane.ny * plane.ny) + plane.nz * plane.nz);
        const double u[3] = {plane.nx / nn, plane.ny / nn, plane.nz / nn};
        const double sgn = a.keep[k] == MM_CLIP_KEEP_BELOW ? 1.0 : -1.0;
        const double step = L ? a.ext_length / (double)L : 0.0;
        for (int64_t j = 1; j <= L; ++j)
            for (int64_t c = c_lo[(size_t)k]; c < c_hi[(size_t)k]; ++c) {
                if (s.kind[(size_t)c] != MM_SECTION_CLOSED) continue;
                for (int64_t i = s.contour_off[(size_t)c]; i < s.contour_off[(size_t)c + 1]; ++i) {
                    for (int d = 0; d < 3; ++d) pl.newv.push_back(s.points[(size_t)(3 * i + d)] + (sgn * ((double)j * step)) * u[d]);
                    pl.new_cut.push_back((int32_t)k);
                }
            }
        const int64_t centres = pl.n_new();
        if (a.cap)
            for (int64_t c = c_lo[(size_t)k]; c < c_hi[(size_t)k]; ++c) {
                if (s.kind[(size_t)c] != MM_SECTION_CLOSED) continue;
                for (int d = 0; d < 3; ++d) {
                    const double x = s.centroid[(size_t)(3 * c + d)];
                    pl.newv.push_back(L ? x + (sgn * ((double)L * step)) * u[d] : x);
                }
                pl.new_cut.push_back((int32_t)k);
            }
        if (pl.n_new() > kMaxIndex) return set_error(MM_ERR_TOO_LARGE, std::string(who) + ": more than 2^31 - 1 new vertices");

        for (int32_t face : faces[(size_t)k]) {
            const int64_t* t = a.f + 3 * (int64_t)face;
            const int s0 = vertex_side(a, plane, t[0]), s1 = vertex_side(a, plane, t[1]), s2 = vertex_side(a, plane, t[2]);
            const int apex = s0 == s1 ? 2 : (s0 == s2 ? 1 : 0);
            const int64_t va = t[apex], vb = t[(apex + 1) % 3], vc = t[(apex + 2) % 3];
            const auto ab = name_of_edge.find(edge_of(va, vb)), ca = name_of_edge.find(edge_of(vc, va));
            if (ab == name_of_edge.end() || ca == name_of_edge.end())
                return set_error(MM_ERR_HIP, std::string(who) + ": a cut face without its loop points");
            Record r;
            std::memset(&r, 0, sizeof(r));
            r.face = face;
            r.cut = (int32_t)k;
            r.flags = apex | (vertex_side(a, plane, va) == a.keep[k] ? clip::kApexKept : 0) | (a.scope[k] == MM_CLIP_SCOPE_LOOP ? clip::kLoopCut : 0);
            r.m_ab = ab->second;
            r.m_ca = ca->second;
            const int32_t kab = crank[(size_t)(r.m_ab - base)], kca = crank[(size_t)(r.m_ca - base)];
            r.r_ab = kab < 0 ? -1 : (int32_t)(ring1 + kab);
            r.r_ca = kca < 0 ? -1 : (int32_t)(ring1 + kca);
            r.ring_stride = (int32_t)closed_points;
            r.centre = -1;
            rec_of[(size_t)face] = (int32_t)pl.rec.size();
            pl.rec.push_back(r);
        }
        // the rim edges of the closed loops, in rim order: edge i leaves point i, the segment of point_face[i]
        int64_t loop = 0, listed = 0;
        for (int64_t c = c_lo[(size_t)k]; c < c_hi[(size_t)k]; ++c) {
            const int64_t lo = s.contour_off[(size_t)c], m = s.contour_off[(size_t)c + 1] - lo;
            if (s.kind[(size_t)c] != MM_SECTION_CLOSED) { ++pl.n_open; listed += m; continue; }
            for (int64_t i = 0; i < m; ++i) {
                const int64_t e = crank[(size_t)(listed + i)];
                const int64_t face = s.point_face[(size_t)(lo + i)];
                if (face < 0 || face >= a.nf || rec_of[(size_t)face] < 0 || pl.rec[(size_t)rec_of[(size_t)face]].cut != k)
                    return set_error(MM_ERR_HIP, std::string(who) + ": a rim edge without its cut face");
                Record& r = pl.rec[(size_t)rec_of[(size_t)face]];
                r.flags |= clip::kClosedRim;
                r.ext_at = (int32_t)(pl.n_ext + 2 * e);
                r.cap_at = (int32_t)(pl.n_cap + e);
                r.centre = a.cap ? (int32_t)(centres + loop) : -1;
                pl.rim.push_back(L ? ring1 + (L - 1) * closed_points + e : base + listed + i);
            }
            pl.rim_off.push_back((int64_t)pl.rim.size());
            listed += m;
            ++loop;
            ++pl.n_closed;
        }
        pl.n_ext += 2 * L * closed_points;
        if (a.cap) pl.n_cap += closed_points;
        if (pl.n_ext + pl.n_cap > kMaxIndex) return set_error(MM_ERR_TOO_LARGE, std::string(who) + ": more than 2^31 - 1 rim faces");
    }
    return MM_OK;
}

void report_sizes(const Args& a, mm_clip_report& rep)
{
    std::memset(&rep, 0, sizeof(rep));
    rep.n_cuts = a.K;
    rep.n_vertices = a.nv;
    rep.n_faces = a.nf;
}

void write_cuts(const Plan& pl, const Args& a, const Out& o)
{
    if (a.K > 0) {
        std::memcpy(o.cut_status, pl.info.data(), (size_t)(4 * a.K) * 8);
        std::memcpy(o.cut_measures, pl.measures.data(), (size_t)(5 * a.K) * 8);
    }
}

// C3: the input mesh with identity maps
int write_identity(const Args& a, const Plan& pl, const Out& o, mm_clip_report& rep, const char* who)
{
    rep.n_vertices = a.nv;
    rep.n_faces = a.nf;
    rep.n_applied = 0;
    if (a.nv > o.vert_cap || a.nf > o.face_cap) {
        *o.report = rep;
        return set_error(MM_ERR_TOO_LARGE, std::string(who) + ": the result passes vert_cap or face_cap");
    }
    if (a.nv > 0) std::memcpy(o.vertices, a.v, (size_t)a.nv * 24);
    if (a.nf > 0) std::memcpy(o.tris, a.f, (size_t)a.nf * 24);
    for (int64_t i = 0; i < a.nv; ++i) o.vertex_origin[i] = i;
    for (int64_t i = 0; i < a.nf; ++i) { o.face_origin[i] = i; o.face_kind[i] = MM_CLIP_KIND_UNTOUCHED; }
    o.rim_off[0] = 0;
    write_cuts(pl, a, o);
    *o.report = rep;
    return MM_OK;
}

void write_rims(const Plan& pl, int64_t kv, const Out& o)
{
    for (size_t i = 0; i < pl.rim_off.size(); ++i) o.rim_off[i] = pl.rim_off[i];
    for (size_t i = 0; i < pl.rim.size(); ++i) o.rim_index[i] = kv + pl.rim[i];
}

void report_plan(const Plan& pl, const Args& a, mm_clip_report& rep)
{
    rep.n_applied = a.K;
    rep.n_new_vertices = pl.n_new();
    rep.n_cut_faces = (int64_t)pl.rec.size();
    rep.n_ext_faces = pl.n_ext;
    rep.n_cap_faces = pl.n_cap;
    rep.n_closed_loops = pl.n_closed;
    rep.n_open_loops = pl.n_open;
}

// C2, C4 and C7 in host C++
int clip_on_host(const Args& a, Plan& pl, const Out& o, mm_clip_report& rep, const char* who)
{
    const int64_t nv = a.nv, nf = a.nf, K = a.K;
    std::vector<int32_t> root((size_t)nv), rec_of((size_t)nf, -1);
    for (int64_t i = 0; i < nv; ++i) root[(size_t)i] = (int32_t)i;
    auto find = [&](int32_t x) { while (root[(size_t)x] != x) { root[(size_t)x] = root[(size_t)root[(size_t)x]]; x = root[(size_t)x]; } return x; };
    auto unite = [&](int64_t p, int64_t q) {
        const int32_t x = find((int32_t)p), y = find((int32_t)q);
        if (x != y) root[(size_t)std::max(x, y)] = std::min(x, y);
    };
    for (size_t r = 0; r < pl.rec.size(); ++r) rec_of[(size_t)pl.rec[r].face] = (int32_t)r;
    for (int64_t i = 0; i < nf; ++i) {
        const int64_t* t = a.f + 3 * i;
        if (rec_of[(size_t)i] < 0) { unite(t[0], t[1]); unite(t[1], t[2]); continue; }
        const int apex = pl.rec[(size_t)rec_of[(size_t)i]].flags & clip::kApexMask;
        unite(t[(apex + 1) % 3], t[(apex + 2) % 3]);
    }
    std::vector<uint8_t> mark((size_t)nv, 0), dropped((size_t)nv, 0);
    for (const Record& r : pl.rec) {
        if (!(r.flags & clip::kLoopCut)) continue;
        const int apex = r.flags & clip::kApexMask;
        const int32_t ra = find((int32_t)a.f[3 * (int64_t)r.face + apex]), rb = find((int32_t)a.f[3 * (int64_t)r.face + (apex + 1) % 3]);
        if (ra == rb) pl.info[(size_t)(4 * r.cut)] = MM_CLIP_NOT_SEPARATING;
        else mark[(size_t)((r.flags & clip::kApexKept) ? rb : ra)] = 1;
    }
    for (int64_t k = 0; k < K; ++k)
        if (pl.info[(size_t)(4 * k)] != MM_CLIP_OK) return write_identity(a, pl, o, rep, who);
    for (int64_t k = 0; k < K; ++k) {
        if (a.scope[k] != MM_CLIP_SCOPE_PLANE) continue;
        const section::Plane plane = plane_of(a, k);
        for (int64_t i = 0; i < nv; ++i)
            if (vertex_side(a, plane, i) != a.keep[k]) dropped[(size_t)i] = 1;
    }
    std::vector<int32_t> vidx((size_t)nv);
    int64_t kv = 0;
    for (int64_t i = 0; i < nv; ++i) {
        if (mark[(size_t)find((int32_t)i)]) dropped[(size_t)i] = 1;
        vidx[(size_t)i] = dropped[(size_t)i] ? -1 : (int32_t)kv++;
    }
    // the orphan check: every status is OK here, so the marks are complete
    bool orphaned = false;
    for (const Record& r : pl.rec) {
        const int64_t* t = a.f + 3 * (int64_t)r.face;
        if (!clip::kept_side_dropped(r.flags, dropped[(size_t)t[0]] != 0, dropped[(size_t)t[1]] != 0, dropped[(size_t)t[2]] != 0)) continue;
        pl.info[(size_t)(4 * r.cut)] = MM_CLIP_KEPT_SIDE_DROPPED;
        orphaned = true;
    }
    if (orphaned) return write_identity(a, pl, o, rep, who);
    // two passes over the faces: the count, then the result
    report_plan(pl, a, rep);
    auto corner = [&](int64_t i) {
        return clip::Corner{vidx[(size_t)i], clip::Point{a.v[3 * i], a.v[3 * i + 1], a.v[3 * i + 2]}, vidx[(size_t)i] < 0};
    };
    auto fresh = [&](int32_t j) {
        return clip::Corner{(int32_t)(kv + j), clip::Point{pl.newv[(size_t)(3 * j)], pl.newv[(size_t)(3 * j + 1)], pl.newv[(size_t)(3 * j + 2)]}, false};
    };
    int64_t kf = 0;
    for (int pass = 0; pass < 2; ++pass) {
        int64_t at = 0;
        auto put = [&](int64_t i0, int64_t i1, int64_t i2, int64_t origin, int kind) {
            if (pass == 1) {
                o.tris[3 * at] = i0; o.tris[3 * at + 1] = i1; o.tris[3 * at + 2] = i2;
                o.face_origin[at] = origin;
                o.face_kind[at] = (int8_t)kind;
            }
            ++at;
        };
        for (int64_t i = 0; i < nf; ++i) {
            const int64_t* t = a.f + 3 * i;
            const int64_t before = at;
            if (rec_of[(size_t)i] < 0) {
                if (!(dropped[(size_t)t[0]] || dropped[(size_t)t[1]] || dropped[(size_t)t[2]]))
                    put(vidx[(size_t)t[0]], vidx[(size_t)t[1]], vidx[(size_t)t[2]], i, MM_CLIP_KIND_UNTOUCHED);
            } else {
                const Record& r = pl.rec[(size_t)rec_of[(size_t)i]];
                const clip::Pieces p = clip::face_pieces(corner(t[0]), corner(t[1]), corner(t[2]), r.flags & clip::kApexMask, fresh(r.m_ab), fresh(r.m_ca));
                for (const clip::Piece* q : {&p.apex, &p.first, &p.second}) {
                    if (!q->kept) continue;
                    put(q->i0, q->i1, q->i2, i, MM_CLIP_KIND_PIECE);
                    if (pass == 0) { ++rep.n_pieces; rep.n_null_pieces += q->null; }
                }
            }
            if (pass == 0 && at == before) ++rep.n_dropped_faces;
        }
        if (pass == 1) break;
        kf = at;
        rep.n_vertices = kv + pl.n_new();
        rep.n_faces = kf + pl.n_ext + pl.n_cap;
        rep.n_dropped_vertices = nv - kv;
        if (rep.n_vertices > kMaxIndex || rep.n_faces > kMaxIndex)
            return set_error(MM_ERR_TOO_LARGE, std::string(who) + ": the result passes 2^31 - 1 vertices or faces");
        if (rep.n_vertices > o.vert_cap || rep.n_faces > o.face_cap) {
            *o.report = rep;
            return set_error(MM_ERR_TOO_LARGE, std::string(who) + ": the result passes vert_cap or face_cap");
        }
    }
    for (int64_t i = 0; i < nv; ++i) {
        if (vidx[(size_t)i] < 0) continue;
        std::memcpy(o.vertices + 3 * (int64_t)vidx[(size_t)i], a.v + 3 * i, 24);
        o.vertex_origin[vidx[(size_t)i]] = i;
    }
    for (int64_t j = 0; j < pl.n_new(); ++j) {
        std::memcpy(o.vertices + 3 * (kv + j), &pl.newv[(size_t)(3 * j)], 24);
        o.vertex_origin[kv + j] = -1 - (int64_t)pl.new_cut[(size_t)j];
    }
    auto store = [&](int64_t at, int64_t i0, int64_t i1, int64_t i2, int64_t cut, int kind) {
        o.tris[3 * at] = kv + i0; o.tris[3 * at + 1] = kv + i1; o.tris[3 * at + 2] = kv + i2;
        o.face_origin[at] = -1 - cut;
        o.face_kind[at] = (int8_t)kind;
    };
    for (const Record& r : pl.rec) {
        if (!(r.flags & clip::kClosedRim)) continue;
        const bool fwd = clip::rim_runs_ab_to_ca(r.flags);
        const int32_t x0 = fwd ? r.m_ab : r.m_ca, y0 = fwd ? r.m_ca : r.m_ab, xr = fwd ? r.r_ab : r.r_ca, yr = fwd ? r.r_ca : r.r_ab;
        auto ring = [&](int32_t rim, int32_t first_ring, int64_t j) { return j == 0 ? (int64_t)rim : (int64_t)first_ring + (j - 1) * r.ring_stride; };
        for (int64_t j = 0; j < a.L; ++j) {
            const int64_t at = kf + r.ext_at + j * 2 * r.ring_stride;
            store(at, ring(y0, yr, j), ring(x0, xr, j), ring(x0, xr, j + 1), r.cut, MM_CLIP_KIND_EXTENSION);
            store(at + 1, ring(y0, yr, j), ring(x0, xr, j + 1), ring(y0, yr, j + 1), r.cut, MM_CLIP_KIND_EXTENSION);
        }
        if (a.cap) store(kf + pl.n_ext + r.cap_at, ring(y0, yr, a.L), ring(x0, xr, a.L), r.centre, r.cut, MM_CLIP_KIND_CAP);
    }
    write_rims(pl, kv, o);
    write_cuts(pl, a, o);
    *o.report = rep;
    return MM_OK;
}

// C2, C4 and C7 on the device: 5 + R launches (R = the jump rounds, the one that changes nothing included), 1 more (the
// orphan check) where no cut is NOT_SEPARATING, and 11 more where the cuts are applied (8 on a mesh without faces, whose
// face scan has no tile)
int clip_on_device(Engine* e, const Args& a, Plan& pl, const Out& o, mm_clip_report& rep, const char* who)
{
    const int64_t nv = a.nv, nf = a.nf, K = a.K, nr = (int64_t)pl.rec.size(), nn = pl.n_new();
    const int64_t v_bound = nv + nn, f_bound = nf + 2 * nr + pl.n_ext + pl.n_cap;
    if (v_bound > kMaxIndex || f_bound > kMaxIndex)
        return set_error(MM_ERR_TOO_LARGE, std::string(who) + ": the result may pass 2^31 - 1 vertices or faces");
    StagedPass sp;
    const size_t o_v = sp.in.take((size_t)nv * 24), o_f = sp.in.take((size_t)nf * 12), o_rec = sp.in.take((size_t)nr * sizeof(Record));
    const size_t o_newv = sp.in.take((size_t)nn * 24), o_newcut = sp.in.take((size_t)nn * 4), o_cuts = sp.in.take((size_t)K * sizeof(ClipCut));
    const size_t o_cnt = sp.out.take(clip_num_counts * 8), o_status = sp.out.take((size_t)K * 4);
    const size_t o_ov = sp.out.take((size_t)v_bound * 24), o_of = sp.out.take((size_t)f_bound * 12), o_vo = sp.out.take((size_t)v_bound * 4);
    const size_t o_fo = sp.out.take((size_t)f_bound * 4), o_fk = sp.out.take((size_t)f_bound);
    const size_t s_link = sp.scratch.take((size_t)nv * 4), s_changed = sp.scratch.take(4), s_frec = sp.scratch.take((size_t)nf * 4);
    const size_t s_mark = sp.scratch.take((size_t)nv), s_vdrop = sp.scratch.take((size_t)nv), s_vkeep = sp.scratch.take((size_t)nv);
    const size_t s_vidx = sp.scratch.take((size_t)nv * 4), s_vtile = sp.scratch.take((clip_scan_tiles(nv) + 1) * 8);
    const size_t s_fcnt = sp.scratch.take((size_t)nf), s_foff = sp.scratch.take((size_t)nf * 4), s_ftile = sp.scratch.take((clip_scan_tiles(nf) + 1) * 8);
    int rc = sp.reserve(e);
    if (rc) return rc;
    std::memcpy(sp.host<double>(o_v), a.v, (size_t)nv * 24);
    narrow_faces(sp.host<int32_t>(o_f), a.f, 3 * nf);
    if (nr) std::memcpy(sp.host<Record>(o_rec), pl.rec.data(), (size_t)nr * sizeof(Record));
    if (nn) {
        std::memcpy(sp.host<double>(o_newv), pl.newv.data(), (size_t)nn * 24);
        std::memcpy(sp.host<int32_t>(o_newcut), pl.new_cut.data(), (size_t)nn * 4);
    }
    for (int64_t k = 0; k < K; ++k) {
        ClipCut c;
        std::memset(&c, 0, sizeof(c));
        std::memcpy(c.o, a.origins + 3 * k, 24);
        std::memcpy(c.n, a.normals + 3 * k, 24);
        c.keep = a.keep[k];
        c.scope = a.scope[k];
        sp.host<ClipCut>(o_cuts)[k] = c;
    }
    MM_TRY_HIP(hipMemcpyAsync(sp.d, sp.h, sp.in.size(), hipMemcpyHostToDevice, e->stream));
    rep.bytes_uploaded = (int64_t)sp.in.size();

    const double* d_v = sp.dev_in<double>(o_v);
    const int32_t* d_f = sp.dev_in<int32_t>(o_f);
    const void* d_rec = sp.dev_in<void>(o_rec);
    unsigned int* d_link = sp.dev_scratch<unsigned int>(s_link);
    uint8_t *d_mark = sp.dev_scratch<uint8_t>(s_mark), *d_vdrop = sp.dev_scratch<uint8_t>(s_vdrop);
    int32_t *d_frec = sp.dev_scratch<int32_t>(s_frec), *d_status = sp.dev_out<int32_t>(o_status);
    unsigned long long* d_counts = sp.dev_out<unsigned long long>(o_cnt);
    int launches = 0;
    MM_TRY_HIP(launch_clip_unions(d_v, nv, d_f, nf, d_rec, nr, sp.dev_in<ClipCut>(o_cuts), (int)K, d_link, d_mark, d_vdrop, d_frec, d_counts,
                                  d_status, &launches, e->stream));
    // the host words of the small reads: the first 256 bytes of the pinned buffer, behind the upload in stream order
    unsigned int* hw = sp.host<unsigned int>(0);
    const int64_t bound = 2 + log2_at_least((unsigned long long)nv) + 8;   // a jumping round halves the depth
    for (;;) {
        MM_TRY_HIP(launch_weld_jump(d_link, nv, sp.dev_scratch<unsigned int>(s_changed), e->stream));
        MM_TRY_HIP(hipMemcpyAsync(hw, sp.dev_scratch<unsigned int>(s_changed), 4, hipMemcpyDeviceToHost, e->stream));
        MM_TRY_HIP(hipStreamSynchronize(e->stream));
        ++rep.jump_rounds;
        ++launches;
        rep.bytes_downloaded += 4;
        if (!hw[0]) break;
        if (rep.jump_rounds > bound) return set_error(MM_ERR_HIP, std::string(who) + ": pointer jumping did not settle");
    }
    MM_TRY_HIP(launch_clip_verdict(d_f, d_rec, nr, d_link, d_mark, d_status, &launches, e->stream));
    std::vector<int32_t> status((size_t)K);
    MM_TRY_HIP(hipMemcpyAsync(status.data(), d_status, (size_t)K * 4, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    rep.bytes_downloaded += K * 4;
    rep.n_launches = launches;
    bool applied = true;
    for (int64_t k = 0; k < K; ++k) {
        if (status[(size_t)k] != 0 && status[(size_t)k] != MM_CLIP_NOT_SEPARATING)
            return set_error(MM_ERR_HIP, std::string(who) + ": cut status out of range");
        if (status[(size_t)k]) { pl.info[(size_t)(4 * k)] = MM_CLIP_NOT_SEPARATING; applied = false; }
    }
    if (!applied) return write_identity(a, pl, o, rep, who);
    // every status word is zero: the marks are complete, and the orphan check can leave nothing but its own value
    MM_TRY_HIP(launch_clip_orphan(d_f, d_rec, nr, d_link, d_mark, d_vdrop, d_status, &launches, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(status.data(), d_status, (size_t)K * 4, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    rep.bytes_downloaded += K * 4;
    rep.n_launches = launches;
    for (int64_t k = 0; k < K; ++k) {
        if (status[(size_t)k] != 0 && status[(size_t)k] != MM_CLIP_KEPT_SIDE_DROPPED)
            return set_error(MM_ERR_HIP, std::string(who) + ": cut status out of range");
        if (status[(size_t)k]) { pl.info[(size_t)(4 * k)] = MM_CLIP_KEPT_SIDE_DROPPED; applied = false; }
    }
    if (!applied) return write_identity(a, pl, o, rep, who);

    int32_t *d_vidx = sp.dev_scratch<int32_t>(s_vidx), *d_foff = sp.dev_scratch<int32_t>(s_foff);
    long long *d_vtile = sp.dev_scratch<long long>(s_vtile), *d_ftile = sp.dev_scratch<long long>(s_ftile);
    uint8_t* d_fcnt = sp.dev_scratch<uint8_t>(s_fcnt);
    MM_TRY_HIP(launch_clip_counts(d_v, nv, sp.dev_in<double>(o_newv), d_f, nf, d_frec, d_rec, d_link, d_mark, d_vdrop,
                                  sp.dev_scratch<uint8_t>(s_vkeep), d_vidx, d_vtile, d_fcnt, d_foff, d_ftile, d_counts, &launches, e->stream));
    long long* ht = sp.host<long long>(0);
    MM_TRY_HIP(hipMemcpyAsync(ht, d_vtile + clip_scan_tiles(nv), 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(ht + 1, d_ftile + clip_scan_tiles(nf), 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    const long long kv = ht[0], kf = ht[1];
    rep.bytes_downloaded += 16;
    if (kv < 0 || kv > nv || kf < 0 || kf > nf + 2 * nr) return set_error(MM_ERR_HIP, std::string(who) + ": compaction count out of range");
    report_plan(pl, a, rep);
    rep.n_vertices = kv + nn;
    rep.n_faces = kf + pl.n_ext + pl.n_cap;
    rep.n_dropped_vertices = nv - kv;
    rep.n_launches = launches;
    if (rep.n_vertices > o.vert_cap || rep.n_faces > o.face_cap) {
        *o.report = rep;
        return set_error(MM_ERR_TOO_LARGE, std::string(who) + ": the result passes vert_cap or face_cap");
    }
    MM_TRY_HIP(launch_clip_emit(d_v, nv, sp.dev_in<double>(o_newv), sp.dev_in<int32_t>(o_newcut), nn, d_f, nf, d_frec, d_rec, nr, d_vidx,
                                kv, d_fcnt, d_foff, (int)a.L, a.cap, kf, kf + pl.n_ext, sp.dev_out<double>(o_ov), sp.dev_out<int32_t>(o_vo),
                                sp.dev_out<int32_t>(o_of), sp.dev_out<int32_t>(o_fo), sp.dev_out<uint8_t>(o_fk), d_counts, &launches, e->stream));
    rep.n_launches = launches;
    const size_t V = (size_t)rep.n_vertices, F = (size_t)rep.n_faces;
    const struct { size_t at, bytes; } down[6] = {{o_cnt, clip_num_counts * 8}, {o_ov, V * 24}, {o_of, F * 12}, {o_vo, V * 4}, {o_fo, F * 4}, {o_fk, F}};
    for (const auto& d : down) {
        if (d.bytes) MM_TRY_HIP(hipMemcpyAsync(sp.host<unsigned char>(d.at), sp.dev_out<unsigned char>(d.at), d.bytes, hipMemcpyDeviceToHost, e->stream));
        rep.bytes_downloaded += (int64_t)d.bytes;
    }
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    const unsigned long long* cnt = sp.host<unsigned long long>(o_cnt);
    if (cnt[clip_num_dropped_faces] > (unsigned long long)nf || cnt[clip_num_untouched] > (unsigned long long)kf ||
        cnt[clip_num_null_pieces] > (unsigned long long)kf)
        return set_error(MM_ERR_HIP, std::string(who) + ": counter out of range");
    rep.n_dropped_faces = (int64_t)cnt[clip_num_dropped_faces];
    rep.n_pieces = kf - (int64_t)cnt[clip_num_untouched];
    rep.n_null_pieces = (int64_t)cnt[clip_num_null_pieces];
    std::memcpy(o.vertices, sp.host<double>(o_ov), V * 24);
    widen_faces(o.tris, sp.host<int32_t>(o_of), 3 * (int64_t)F);
    for (size_t i = 0; i < V; ++i) o.vertex_origin[i] = sp.host<int32_t>(o_vo)[i];
    for (size_t i = 0; i < F; ++i) { o.face_origin[i] = sp.host<int32_t>(o_fo)[i]; o.face_kind[i] = (int8_t)sp.host<uint8_t>(o_fk)[i]; }
    write_rims(pl, kv, o);
    write_cuts(pl, a, o);
    *o.report = rep;
    return MM_OK;
}

int clip_mesh(mm_engine* h, bool on_device, const Args& a, const Out& o, const char* who)
{
    Engine* e = nullptr;
    int rc;
    if (on_device && (rc = engine_of(h, e))) return rc;
    if ((rc = check_args(a, o, who))) return rc;
    mm_clip_report rep;
    report_sizes(a, rep);
    Sections s;
    Plan pl;
    if (a.K > 0) {
        if ((rc = on_device ? sections_on_device(h, a, s) : sections_on_host(a, s))) return rc;
        if ((rc = build_plan(a, s, who, pl))) return rc;
    } else {
        pl.rim_off.assign(1, 0);
    }
    // without a cut or with a status C1 set there is nothing to decide; without a vertex nothing for the device to do
    if (a.K == 0 || !pl.ok) return write_identity(a, pl, o, rep, who);
    return on_device && a.nv > 0 ? clip_on_device(e, a, pl, o, rep, who) : clip_on_host(a, pl, o, rep, who);
}

}  // namespace

extern "C" {

int mm_mesh_clip(mm_engine* e, const double* v, int64_t nv, const int64_t* tris, int64_t nf, const double* origins,
                 const double* normals, const int32_t* keep, const int32_t* scope, int64_t n_cuts, int32_t cap, double ext_length,
                 int64_t ext_layers, int64_t vert_cap, int64_t face_cap, double* out_vertices, int64_t* out_tris,
                 int64_t* vertex_origin, int64_t* face_origin, int8_t* face_kind, int64_t* cut_status, double* cut_measures,
                 int64_t* rim_off, int64_t* rim_index, mm_clip_report* report)
{
    return clip_mesh(e, true, Args{v, nv, tris, nf, origins, normals, keep, scope, n_cuts, cap, ext_length, ext_layers},
                Out{vert_cap, face_cap, out_vertices, out_tris, vertex_origin, face_origin, face_kind, cut_status, cut_measures, rim_off,
                    rim_index, report}, "mm_mesh_clip");
}

int mm_mesh_clip_host(const double* v, int64_t nv, const int64_t* tris, int64_t nf, const double* origins, const double* normals,
                      const int32_t* keep, const int32_t* scope, int64_t n_cuts, int32_t cap, double ext_length, int64_t ext_layers,
                      int64_t vert_cap, int64_t face_cap, double* out_vertices, int64_t* out_tris, int64_t* vertex_origin,
                      int64_t* face_origin, int8_t* face_kind, int64_t* cut_status, double* cut_measures, int64_t* rim_off,
                      int64_t* rim_index, mm_clip_report* report)
{
    return clip_mesh(nullptr, false, Args{v, nv, tris, nf, origins, normals, keep, scope, n_cuts, cap, ext_length, ext_layers},
                Out{vert_cap, face_cap, out_vertices, out_tris, vertex_origin, face_origin, face_kind, cut_status, cut_measures, rim_off,
                    rim_index, report}, "mm_mesh_clip_host");
}

}  // extern "C"
