// mm_stitch.cpp -- CCTA stitching (include/mm_ccta.h): the seam between a trimmed CCTA mesh and the intravascular lumen,
// and the assembly of the joined mesh.  Reference: multimodars/ccta/stitching.py:69-107 (rings to ends), :355-481
// (stitch_ccta_to_intravascular), :1148-1334 (ring start, ring direction, the strip), multimodars/_converters.py:
// 1018-1085 (the IV tube), src/ccta/binding/ccta_py.rs:596-700 (fix_mesh_winding).  What runs over every vertex and face
// of the joined mesh -- weld, repeated and degenerate faces, winding, inversion -- runs on the device
// (mm_weld_kernels.hip); the seam touches a few hundred points and is host C++ here.
//
// The winding stage is a union-find with the parity beside the parent link: one lock-free hook launch, then pointer
// jumping until no link moves.  Every jump round at least halves the depth of every face below its root, which is below
// the face count, so the stage takes at most 2 + ceil(log2(max(nf, 2))) launches whatever the mesh's diameter.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/mm_ccta.h"
#include "mm_stage.h"

namespace mm {
namespace {

// ---- the seam (host) ------------------------------------------------------------------------------------------------

inline double norm3(double x, double y, double z) { return std::sqrt((x * x + y * y) + z * z); }

inline double dist3(const double* a, const double* b) { return norm3(a[0] - b[0], a[1] - b[1], a[2] - b[2]); }

// _newell_normal (stitching.py:1194-1210)
void newell_normal(const double* p, int64_t n, double out[3])
{
    double nx = 0.0, ny = 0.0, nz = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        const double* c = p + 3 * i;
        const double* x = p + 3 * ((i + 1) % n);
        nx += (c[1] - x[1]) * (c[2] + x[2]);
        ny += (c[2] - x[2]) * (c[0] + x[0]);
        nz += (c[0] - x[0]) * (c[1] + x[1]);
    }
    const double len = norm3(nx, ny, nz);
    if (len > 1e-10) { out[0] = nx / len; out[1] = ny / len; out[2] = nz / len; }
    else { out[0] = 0.0; out[1] = 0.0; out[2] = 1.0; }
}

inline void cross3(const double* a, const double* b, double out[3])
{
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}

inline double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// _signed_area_projected (stitching.py:1176-1191)
double signed_area_projected(const double* p, int64_t n, const double normal[3])
{
    const double ref_x[3] = {1.0, 0.0, 0.0}, ref_y[3] = {0.0, 1.0, 0.0};
    double u[3], v[3];
    cross3(normal, std::fabs(normal[0]) < 0.9 ? ref_x : ref_y, u);
    const double ul = norm3(u[0], u[1], u[2]);
    u[0] /= ul; u[1] /= ul; u[2] /= ul;
    cross3(normal, u, v);
    double sum = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        const double* a = p + 3 * i;
        const double* b = p + 3 * ((i + 1) % n);
        sum += dot3(a, u) * dot3(b, v) - dot3(b, u) * dot3(a, v);
    }
    return 0.5 * sum;
}

// summed distance of ring point i (order: 0, then forwards or backwards) to IV point i * step, over the first m
double total_dist(const double* ring, int64_t n_b, bool reversed, const double* iv, int64_t step, int64_t m)
{
    double sum = 0.0;
    for (int64_t i = 0; i < m; ++i) {
        const int64_t k = (reversed && i > 0) ? n_b - i : i;
        sum += dist3(ring + 3 * k, iv + 3 * i * step);
    }
    return sum;
}

inline void reverse_faces(int64_t* faces, int64_t nf)
{
    for (int64_t f = 0; f < nf; ++f) std::swap(faces[3 * f], faces[3 * f + 2]);
}

// ---- device part -----------------------------------------------------------------------------------------------------

// The device buffers of one assembly, carved out of the engine's grow-only device buffer.
struct WeldDev {
    int32_t *face = nullptr, *table = nullptr, *rep = nullptr, *vidx = nullptr, *vmap = nullptr, *frep = nullptr,
            *fidx = nullptr, *out_f = nullptr;
    double *vert = nullptr, *out_v = nullptr, *sum_a = nullptr, *sum_b = nullptr, *volume = nullptr;
    uint8_t *ref = nullptr, *keep = nullptr, *fkeep = nullptr;
    long long *vtile = nullptr, *ftile = nullptr;
    EdgeTable edges;
    unsigned long long* counts = nullptr;    // unreferenced, degenerate, repeated, flipped, open, non-manifold, conflicts
    unsigned int *link = nullptr, *changed = nullptr;
    int log2_v = 8, log2_f = 8;
};

enum { kUnref = 0, kDegenerate = 1, kRepeated = 2, kFlipped = 3, kOpen = 4, kNonManifold = 5, kConflict = 6, kCounts = 8 };

// winding of the nf faces at `face` (device, in place): the edge table, the union-find, the flips and the edge report
int wind(Engine* e, WeldDev& d, int32_t* face, int64_t nf, bool fix, int64_t* rounds)
{
    const EdgeTable& t = d.edges;
    const WindDev w{t.keys, t.cnt, t.own, d.link, d.changed, d.counts + kFlipped, d.counts + kOpen, t.log2_e};
    return weld_wind(e, w, face, nf, fix, rounds);
}

}  // namespace

int weld_wind(Engine* e, const WindDev& d, int32_t* face, int64_t nf, bool fix, int64_t* rounds)
{
    *rounds = 0;
    MM_TRY_HIP(launch_weld_edges(face, nf, d.keys, d.cnt, d.own, d.log2_e, e->stream));
    if (fix && nf > 0) {
        MM_TRY_HIP(launch_weld_hook(d.keys, d.cnt, d.own, d.log2_e, d.link, nf, e->stream));
        *rounds = 1;
        unsigned int* hc = (unsigned int*)e->host_pts.p;
        const int64_t bound = 2 + log2_at_least((unsigned long long)nf) + 8;          // never reached: see the header
        for (;;) {
            MM_TRY_HIP(launch_weld_jump(d.link, nf, d.changed, e->stream));
            MM_TRY_HIP(hipMemcpyAsync(hc, d.changed, 4, hipMemcpyDeviceToHost, e->stream));
            MM_TRY_HIP(hipStreamSynchronize(e->stream));
            ++*rounds;
            if (!hc[0]) break;
            if (*rounds > bound) return set_error(MM_ERR_HIP, "winding: pointer jumping did not settle");
        }
        MM_TRY_HIP(launch_weld_flip(face, nf, d.link, d.n_flipped, e->stream));
    }
    MM_TRY_HIP(launch_weld_edge_report(d.keys, d.cnt, d.own, d.log2_e, fix && nf > 0 ? d.link : nullptr,
                                       d.edge_counts, e->stream));
    return MM_OK;
}

}  // namespace mm

using namespace mm;

extern "C" {

int mm_fix_winding(mm_engine* h, const int64_t* faces, int64_t nf, int64_t* out_faces, int64_t* info)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (nf < 0 || nf > kMaxIndex || !info || (nf > 0 && (!faces || !out_faces)))
        return set_error(MM_ERR_INVALID, "mm_fix_winding: bad arguments");
    if ((rc = faces_in_range(faces, nf, kMaxIndex + 1, "mm_fix_winding"))) return rc;   // no nv: what an int32 holds
    std::memset(info, 0, 3 * sizeof(int64_t));
    if (nf == 0) return MM_OK;
    WeldDev d;
    if ((rc = e->ensure(e->host_pts, (size_t)nf * 12 + 256, true))) return rc;
    rc = carve_on(e, e->dev_pts, [&](Carve& c) {
        c.place(d.face, 3 * (size_t)nf);
        d.edges.lay(c, nf);
        c.place(d.link, (size_t)nf); c.place(d.counts, kCounts); c.place(d.changed, 1);
    });
    if (rc) return rc;
    int32_t* hf = (int32_t*)e->host_pts.p;
    narrow_faces(hf, faces, 3 * nf);
    MM_TRY_HIP(hipMemcpyAsync(d.face, hf, (size_t)nf * 12, hipMemcpyHostToDevice, e->stream));
    MM_TRY_HIP(hipMemsetAsync(d.counts, 0, kCounts * 8, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));                        // the pinned buffer takes the round flags next
    int64_t rounds = 0;
    if ((rc = wind(e, d, d.face, nf, true, &rounds))) return rc;
    unsigned long long* hcnt = (unsigned long long*)((unsigned char*)e->host_pts.p + up256((size_t)nf * 12));
    MM_TRY_HIP(hipMemcpyAsync(hf, d.face, (size_t)nf * 12, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(hcnt, d.counts, kCounts * 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    widen_faces(out_faces, hf, 3 * nf);
    info[0] = (int64_t)hcnt[kFlipped];
    info[1] = (int64_t)hcnt[kConflict];
    info[2] = rounds;
    return MM_OK;
}

int mm_mesh_assemble(mm_engine* h, int n_parts, const double* vertices_xyz, const int64_t* vert_off,
                     const int64_t* faces, const int64_t* face_off, int merge_digits, int fix_winding, int fix_inversion,
                     double* out_vertices, int64_t* out_faces, mm_assemble_report* report)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (n_parts < 0 || !report || (n_parts > 0 && (!vert_off || !face_off)) || merge_digits < 0 || merge_digits > 15 ||
        (fix_winding != 0 && fix_winding != 1) || (fix_inversion != 0 && fix_inversion != 1))
        return set_error(MM_ERR_INVALID, "mm_mesh_assemble: bad arguments");
    std::memset(report, 0, sizeof(*report));
    if (n_parts == 0) return MM_OK;
    if (vert_off[0] != 0 || face_off[0] != 0) return set_error(MM_ERR_INVALID, "mm_mesh_assemble: offsets must start at 0");
    for (int p = 0; p < n_parts; ++p)
        if (vert_off[p + 1] < vert_off[p] || face_off[p + 1] < face_off[p] || vert_off[p + 1] > kMaxIndex ||
            face_off[p + 1] > kMaxIndex)
            return set_error(MM_ERR_INVALID, "mm_mesh_assemble: offsets must ascend and stay below 2^31");
    const int64_t nv = vert_off[n_parts], nf = face_off[n_parts];
    if ((nv > 0 && (!vertices_xyz || !out_vertices)) || (nf > 0 && (!faces || !out_faces)))
        return set_error(MM_ERR_INVALID, "mm_mesh_assemble: bad arguments");
    for (int p = 0; p < n_parts; ++p)
        if ((rc = faces_in_range(faces + 3 * face_off[p], face_off[p + 1] - face_off[p], vert_off[p + 1] - vert_off[p],
                                 "mm_mesh_assemble")))
            return rc;
    if (nf == 0) { report->n_unreferenced_vertices = nv; return MM_OK; }   // no face names a vertex

    double scale = 1.0;
    for (int k = 0; k < merge_digits; ++k) scale *= 10.0;              // exact: 10^15 < 2^53

    WeldDev d;
    d.log2_v = log2_at_least(2ull * (unsigned long long)nv);
    d.log2_f = log2_at_least(2ull * (unsigned long long)nf);
    const size_t cap_t = (size_t)1 << std::max(d.log2_v, d.log2_f), V = (size_t)nv, Fn = (size_t)nf;
    size_t o_vert = 0, in_bytes = 0;
    rc = carve_on(e, e->dev_pts, [&](Carve& c) {
        c.place(d.face, 3 * Fn); o_vert = c.place(d.vert, 3 * V);
        in_bytes = c.size();
        c.place(d.ref, V); c.place(d.keep, V); c.place(d.rep, V);
        c.place(d.vidx, V); c.place(d.vmap, V); c.place(d.vtile, trim_scan_tiles(nv) + 1);
        c.place(d.table, cap_t); c.place(d.frep, Fn); c.place(d.fkeep, Fn);
        c.place(d.fidx, Fn); c.place(d.ftile, trim_scan_tiles(nf) + 1);
        c.place(d.out_v, 3 * V); c.place(d.out_f, 3 * Fn);
        d.edges.lay(c, nf);
        c.place(d.link, Fn);
        c.place(d.sum_a, Fn); c.place(d.sum_b, weld_sum_scratch(nf)); c.place(d.volume, 1);
        c.place(d.counts, kCounts); c.place(d.changed, 1);
    });
    if (rc) return rc;
    if ((rc = e->ensure(e->host_pts, std::max(in_bytes, V * 24 + Fn * 12 + 512), true))) return rc;
    unsigned char* hb = (unsigned char*)e->host_pts.p;
    int32_t* hf = (int32_t*)hb;
    for (int p = 0; p < n_parts; ++p)
        narrow_faces(hf + 3 * face_off[p], faces + 3 * face_off[p], 3 * (face_off[p + 1] - face_off[p]), vert_off[p]);
    if (nv > 0) std::memcpy(hb + o_vert, vertices_xyz, V * 24);

    MM_TRY_HIP(hipMemcpyAsync(d.face, hb, in_bytes, hipMemcpyHostToDevice, e->stream));
    MM_TRY_HIP(hipMemsetAsync(d.counts, 0, kCounts * 8, e->stream));
    MM_TRY_HIP(hipMemsetAsync(d.volume, 0, 8, e->stream));
    MM_TRY_HIP(launch_weld_vertices(d.vert, nv, d.face, nf, scale, d.ref, d.table, d.log2_v, d.rep, d.keep,
                                    d.counts + kUnref, e->stream));
    MM_TRY_HIP(launch_trim_scan(d.keep, nv, d.vtile, d.vidx, e->stream));
    MM_TRY_HIP(launch_weld_faces(d.face, nf, nv, d.rep, d.vidx, d.vmap, d.table, d.log2_f, d.frep, d.fkeep,
                                 d.counts + kDegenerate, e->stream));
    MM_TRY_HIP(launch_trim_scan(d.fkeep, nf, d.ftile, d.fidx, e->stream));
    MM_TRY_HIP(launch_trim_compact(d.vert, nv, d.vidx, d.face, 0, d.fidx, d.out_v, d.out_f, e->stream));   // vertices
    MM_TRY_HIP(launch_trim_compact(d.vert, 0, d.vmap, d.face, nf, d.fidx, d.out_v, d.out_f, e->stream));    // faces
    long long kv, kf;
    if ((rc = scan_totals(e, d.vtile, nv, d.ftile, nf, &kv, &kf, "mm_mesh_assemble"))) return rc;

    int64_t rounds = 0;
    if ((rc = wind(e, d, d.out_f, kf, fix_winding != 0, &rounds))) return rc;
    double volume = 0.0;
    int inverted = 0;
    if (fix_inversion) {
        MM_TRY_HIP(launch_weld_volume(d.out_v, d.out_f, kf, d.sum_a, d.sum_b, d.volume, e->stream));
        double* hv = (double*)hb;
        MM_TRY_HIP(hipMemcpyAsync(hv, d.volume, 8, hipMemcpyDeviceToHost, e->stream));
        MM_TRY_HIP(hipStreamSynchronize(e->stream));
        volume = hv[0] / 6.0;
        if (volume < 0.0) {
            inverted = 1;
            MM_TRY_HIP(launch_weld_reverse(d.out_f, kf, e->stream));
        }
    }
    const size_t h_faces = up256((size_t)kv * 24), h_counts = up256(h_faces + (size_t)kf * 12);
    if (kv) MM_TRY_HIP(hipMemcpyAsync(hb, d.out_v, (size_t)kv * 24, hipMemcpyDeviceToHost, e->stream));
    if (kf) MM_TRY_HIP(hipMemcpyAsync(hb + h_faces, d.out_f, (size_t)kf * 12, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(hb + h_counts, d.counts, kCounts * 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    std::memcpy(out_vertices, hb, (size_t)kv * 24);
    const int32_t* f32 = (const int32_t*)(hb + h_faces);
    widen_faces(out_faces, f32, 3 * kf);
    const unsigned long long* c = (const unsigned long long*)(hb + h_counts);
    report->n_vertices = kv;
    report->n_faces = kf;
    report->n_unreferenced_vertices = (int64_t)c[kUnref];
    report->n_welded_vertices = nv - (int64_t)c[kUnref] - kv;
    report->n_degenerate_faces = (int64_t)c[kDegenerate];
    report->n_duplicate_faces = (int64_t)c[kRepeated];
    report->n_flipped_faces = (int64_t)c[kFlipped];
    report->n_winding_conflicts = (int64_t)c[kConflict];
    report->n_open_edges = (int64_t)c[kOpen];
    report->n_nonmanifold_edges = (int64_t)c[kNonManifold];
    report->inverted = inverted;
    report->winding_rounds = rounds;
    report->volume = volume;
    return MM_OK;
}

int mm_assign_rings_to_ends(const double* rings_xyz, const int64_t* ring_off, int64_t n_rings, const double prox[3],
                            const double dist[3], int64_t pair[2])
{
    if (n_rings < 2 || !rings_xyz || !ring_off || !prox || !dist || !pair)
        return set_error(MM_ERR_INVALID, "mm_assign_rings_to_ends: bad arguments");
    std::vector<double> c((size_t)n_rings * 3);
    for (int64_t r = 0; r < n_rings; ++r) {
        const int64_t n = ring_off[r + 1] - ring_off[r];
        if (n < 1 || ring_off[r] < 0) return set_error(MM_ERR_INVALID, "mm_assign_rings_to_ends: empty ring");
        double s[3] = {0.0, 0.0, 0.0};
        for (int64_t i = ring_off[r]; i < ring_off[r + 1]; ++i)
            for (int k = 0; k < 3; ++k) s[k] += rings_xyz[3 * i + k];
        for (int k = 0; k < 3; ++k) c[3 * r + k] = s[k] / (double)n;
    }
    double best = INFINITY;
    pair[0] = 0;
    pair[1] = 1;
    for (int64_t i = 0; i < n_rings; ++i)
        for (int64_t j = 0; j < n_rings; ++j) {
            if (i == j) continue;
            const double cost = dist3(&c[3 * i], prox) + dist3(&c[3 * j], dist);
            if (cost < best) { best = cost; pair[0] = i; pair[1] = j; }
        }
    return MM_OK;
}

int64_t mm_ring_start(const double* ring_xyz, int64_t n, int mode, const double* iv_pt)
{
    if (n < 1 || !ring_xyz || (mode != 0 && mode != 1) || (mode == 0 && !iv_pt))
        return set_error(MM_ERR_INVALID, "mm_ring_start: bad arguments");
    int64_t best = 0;
    double bv = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        const double v = mode == 0 ? dist3(ring_xyz + 3 * i, iv_pt) : ring_xyz[3 * i + 2];
        if (std::isnan(v)) return i;
        if (i == 0 || (mode == 0 ? v < bv : v > bv)) { bv = v; best = i; }
    }
    return best;
}

int mm_ring_direction(const double* ring_xyz, int64_t n_b, const double* iv_xyz, int64_t n_iv, int mode,
                      int64_t point_step)
{
    if (n_b < 1 || n_iv < 1 || !ring_xyz || !iv_xyz || (mode != 0 && mode != 1) || (mode == 0 && point_step < 1))
        return set_error(MM_ERR_INVALID, "mm_ring_direction: bad arguments");
    if (mode == 0) {
        const int64_t n_sub = (n_iv + point_step - 1) / point_step;     // iv_pts[0::step]
        const int64_t m = std::min(n_b, n_sub);
        return total_dist(ring_xyz, n_b, true, iv_xyz, point_step, m) < total_dist(ring_xyz, n_b, false, iv_xyz, point_step, m)
                   ? 1 : 0;
    }
    double normal[3];
    newell_normal(iv_xyz, n_iv, normal);
    return signed_area_projected(ring_xyz, n_b, normal) < 0.0 ? 1 : 0;
}

int mm_stitch_rings(const double* ring_xyz, int64_t n_b, const double* iv_xyz, int64_t n_iv, const double* outward,
                    int64_t* faces)
{
    if (n_b < 3 || n_iv < 3 || !ring_xyz || !iv_xyz || !faces)
        return set_error(MM_ERR_INVALID, "mm_stitch_rings: need at least 3 points per ring");
    int64_t i = 0, j = 0, f = 0;
    while (i < n_b || j < n_iv) {
        const bool take_boundary = j >= n_iv || (i < n_b && (double)(i + 1) / (double)n_b <= (double)(j + 1) / (double)n_iv);
        if (take_boundary) {
            faces[3 * f] = i % n_b; faces[3 * f + 1] = (i + 1) % n_b; faces[3 * f + 2] = n_b + j % n_iv;
            ++i;
        } else {
            faces[3 * f] = i % n_b; faces[3 * f + 1] = n_b + (j + 1) % n_iv; faces[3 * f + 2] = n_b + j % n_iv;
            ++j;
        }
        ++f;
    }
    if (!outward) return 0;
    auto at = [&](int64_t k) { return k < n_b ? ring_xyz + 3 * k : iv_xyz + 3 * (k - n_b); };
    double s[3] = {0.0, 0.0, 0.0};
    int64_t valid = 0;
    for (int64_t k = 0; k < f; ++k) {
        const double *p0 = at(faces[3 * k]), *p1 = at(faces[3 * k + 1]), *p2 = at(faces[3 * k + 2]);
        const double e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
        const double e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
        double n[3];
        cross3(e1, e2, n);
        const double len = norm3(n[0], n[1], n[2]);
        const double u[3] = {n[0] / len, n[1] / len, n[2] / len};
        if (!std::isfinite(u[0]) || !std::isfinite(u[1]) || !std::isfinite(u[2])) continue;
        s[0] += u[0]; s[1] += u[1]; s[2] += u[2];
        ++valid;
    }
    if (valid == 0) return 0;
    const double mean[3] = {s[0] / (double)valid, s[1] / (double)valid, s[2] / (double)valid};
    if (dot3(mean, outward) < 0.0) { reverse_faces(faces, f); return 1; }
    return 0;
}

int mm_tube_faces(const double* contours_xyz, int64_t n_contours, int64_t n_points, const double centroid0[3],
                  int64_t* faces)
{
    if (n_contours < 2 || n_points < 1 || !contours_xyz || !centroid0 || !faces ||
        n_contours > kMaxIndex / n_points)
        return set_error(MM_ERR_INVALID, "mm_tube_faces: need at least two contours");
    int64_t f = 0;
    for (int64_t i = 0; i + 1 < n_contours; ++i)
        for (int64_t j = 0; j < n_points; ++j) {
            const int64_t j1 = (j + 1) % n_points;
            const int64_t a = i * n_points + j, b = i * n_points + j1, c = (i + 1) * n_points + j1, dd = (i + 1) * n_points + j;
            faces[3 * f] = a; faces[3 * f + 1] = b; faces[3 * f + 2] = dd; ++f;
            faces[3 * f] = b; faces[3 * f + 1] = c; faces[3 * f + 2] = dd; ++f;
        }
    const double *p0 = contours_xyz + 3 * faces[0], *p1 = contours_xyz + 3 * faces[1], *p2 = contours_xyz + 3 * faces[2];
    const double e1[3] = {p1[0] - p0[0], p1[1] - p0[1], p1[2] - p0[2]};
    const double e2[3] = {p2[0] - p0[0], p2[1] - p0[1], p2[2] - p0[2]};
    double n[3];
    cross3(e1, e2, n);
    const double to[3] = {((p0[0] + p1[0]) + p2[0]) / 3.0 - centroid0[0], ((p0[1] + p1[1]) + p2[1]) / 3.0 - centroid0[1],
                          ((p0[2] + p1[2]) + p2[2]) / 3.0 - centroid0[2]};
    if (dot3(n, to) < 0.0) { reverse_faces(faces, f); return 1; }
    return 0;
}

}  // extern "C"
