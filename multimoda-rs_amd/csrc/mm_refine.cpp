// mm_refine.cpp -- CCTA mesh refinement (include/mm_ccta.h, "mesh refinement"): long edges split at their midpoint, pass
// after pass, and the edge lengths that choose the target.  Reference: multimodars/ccta/fixing_functions.py:114-239 (the
// isotropic remesh of fix_and_remesh_stitched_mesh, of which this is the edge split alone).  The host checks the
// arguments, narrows the triangles to int32, sizes the buffers from the counters each pass reads back and fills the
// report; everything over the mesh runs on the device (mm_refine_kernels.hip, the volume of mm_weld_kernels.hip).
//
// The mesh lives in one block, [vertices | parents of the new vertices | faces], in e->dev_pts and e->dev_lvl by turns: a
// pass reads one and writes the other, grown to the sizes its scan found.  What a pass needs beside the mesh (the edge
// table, the corners' slots, the codes, the offsets, the counters, the volume's scratch) is carved from e->dev_raw, sized
// by the faces the pass reads.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>

#include "../../include/mm_ccta.h"
#include "mm_mesh_layout.h"

namespace mm {
namespace {

// words of the counters block: those of mm_refine_kernels.hip, then the volume
enum { kEdges = 0, kOpen, kNonManifold, kLongest, kMarked, kOne, kTwo, kThree, kNewVerts, kChildren, kVolume,
       kWords = kRefineWords };

// one generation of the mesh on the device
struct Block {
    int64_t nv, nf, nv0;
    size_t o_par() const { return (size_t)nv * 24; }
    size_t o_face() const { return o_par() + (size_t)(nv - nv0) * 8; }
    size_t bytes() const { return o_face() + (size_t)nf * 12; }
};

// the edges of one generation, as its marks counted them
struct EdgeStats {
    int64_t edges = 0, open = 0, nonmanifold = 0;
    double longest_sq = 0.0;
    void read(const unsigned long long* c)
    {
        edges = (int64_t)c[kEdges]; open = (int64_t)c[kOpen]; nonmanifold = (int64_t)c[kNonManifold];
        std::memcpy(&longest_sq, &c[kLongest], 8);
    }
};

// the front of a pass over the mesh at `b`: the edge table and the marks, with `counts` the faces' codes and the scan of
// their tile sums; the counters come back through the first words of e->host_pts (behind the upload in stream order)
int pass_front(Engine* e, const RefineScratch& s, const Block& m, const unsigned char* b, double thr2, int all, bool counts,
               int64_t* launches, const unsigned long long** words)
{
    const double* v = (const double*)b;
    const int32_t* face = (const int32_t*)(b + m.o_face());
    MM_TRY_HIP(launch_refine_edges(face, m.nf, s.t.keys, s.t.cnt, s.t.own, s.t.log2_e, s.slot, e->stream));
    MM_TRY_HIP(launch_refine_marks(s.t.keys, s.t.cnt, s.t.own, s.t.log2_e, v, thr2, all, s.counts, e->stream));
    *launches += 2;
    if (counts) {
        MM_TRY_HIP(launch_refine_counts(s.slot, s.t.own, m.nf, s.code, s.tile, s.counts, e->stream));
        *launches += 2;
    }
    return read_words(e, s.counts, kWords, words);
}

}  // namespace
}  // namespace mm

using namespace mm;

extern "C" {

int mm_mesh_edge_lengths(mm_engine* h, const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf,
                         int64_t edge_cap, int64_t* out_edges, double* out_len_sq, int64_t* info)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (!info || edge_cap < 0 || (edge_cap > 0 && (!out_edges || !out_len_sq)))
        return set_error(MM_ERR_INVALID, "mm_mesh_edge_lengths: bad arguments");
    if ((rc = mesh_args("mm_mesh_edge_lengths", vertices_xyz, nv, tris, nf, true))) return rc;
    std::memset(info, 0, 4 * sizeof(int64_t));
    if (nv == 0 || nf == 0) return MM_OK;
    MeshUp up;
    if ((rc = mesh_upload(e, vertices_xyz, nv, tris, nf, nullptr, 0, up))) return rc;
    const Block m{nv, nf, nv};
    RefineScratch s;
    const size_t o_len = up256((size_t)nf * 24);                       // at most 3 nf edges: int32 pairs, then doubles
    if ((rc = carve_on(e, e->dev_raw, [&](Carve& c) { s.lay(c, nf, o_len + (size_t)nf * 24); }))) return rc;
    const unsigned char* b = (const unsigned char*)e->dev_pts.p;
    int64_t launches = 0;
    const unsigned long long* c;
    if ((rc = pass_front(e, s, m, b, 0.0, 1, true, &launches, &c))) return rc;
    const int64_t n = (int64_t)c[kNewVerts];
    if (n != (int64_t)c[kMarked] || n != (int64_t)c[kEdges] || n > 3 * nf)
        return set_error(MM_ERR_HIP, "mm_mesh_edge_lengths: the scan and the edge count disagree");
    info[0] = n; info[1] = (int64_t)c[kOpen]; info[2] = (int64_t)c[kNonManifold]; info[3] = launches;
    if (n > edge_cap) return set_error(MM_ERR_TOO_LARGE, "mm_mesh_edge_lengths: edge_cap too small (info[0] holds the size)");
    if (n == 0) return MM_OK;
    MM_TRY_HIP(launch_refine_edge_list(s.code, nf, s.tile, s.slot, s.t.keys, (const double*)b, (int32_t*)s.list,
                                       (double*)(s.list + o_len), e->stream));
    info[3] = ++launches;
    const size_t h_len = up256((size_t)n * 8);
    if ((rc = e->ensure(e->host_pts, h_len + (size_t)n * 8 + 512, true))) return rc;
    unsigned char* hb = (unsigned char*)e->host_pts.p;
    MM_TRY_HIP(hipMemcpyAsync(hb, s.list, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(hb + h_len, s.list + o_len, (size_t)n * 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    widen_faces(out_edges, (const int32_t*)hb, 2 * n);
    std::memcpy(out_len_sq, hb + h_len, (size_t)n * 8);
    return MM_OK;
}

int mm_mesh_refine(mm_engine* h, const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf, double target_len,
                   double ratio, int64_t max_passes, int64_t max_vertices, int64_t vert_cap, int64_t face_cap,
                   double* out_vertices, int64_t* out_tris, int64_t* out_parents, mm_refine_report* report)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    const double thr = ratio * target_len, thr2 = thr * thr;
    if (!report || max_passes < 0 || max_vertices < 0 || vert_cap < 0 || face_cap < 0 || !(target_len > 0.0) ||
        !(ratio > 0.0) || !std::isfinite(thr2) || !(thr2 > 0.0) || (vert_cap > 0 && !out_vertices) ||
        (face_cap > 0 && !out_tris) || (nv >= 0 && vert_cap > nv && !out_parents))
        return set_error(MM_ERR_INVALID, "mm_mesh_refine: bad arguments");
    if ((rc = mesh_args("mm_mesh_refine", vertices_xyz, nv, tris, nf, true))) return rc;
    std::memset(report, 0, sizeof(*report));
    report->n_vertices = nv;
    report->n_faces = nf;
    if (nv == 0 || nf == 0) {                                          // no edge: nothing to split
        if (vert_cap < nv || face_cap < nf)
            return set_error(MM_ERR_TOO_LARGE, "mm_mesh_refine: vert_cap / face_cap too small (the report holds the sizes)");
        if (nv > 0) std::memcpy(out_vertices, vertices_xyz, (size_t)nv * 24);
        if (nf > 0) std::memcpy(out_tris, tris, (size_t)nf * 24);
        return MM_OK;
    }
    MeshUp up;
    if ((rc = mesh_upload(e, vertices_xyz, nv, tris, nf, nullptr, 0, up))) return rc;
    report->bytes_uploaded = (int64_t)up.up_bytes;

    Engine::Buf* cur = &e->dev_pts;
    Engine::Buf* oth = &e->dev_lvl;
    Block m{nv, nf, nv};
    RefineScratch s;
    EdgeStats before, after;
    int64_t launches = 0, passes = 0;
    for (bool first = true;; first = false) {
        if ((rc = carve_on(e, e->dev_raw, [&](Carve& c) { s.lay(c, m.nf); }))) return rc;
        unsigned char* b = (unsigned char*)cur->p;
        if (first) {
            MM_TRY_HIP(launch_weld_volume((const double*)b, (const int32_t*)(b + m.o_face()), m.nf, s.sa, s.sb,
                                          (double*)(s.counts + kVolume), e->stream));
            launches += weld_volume_launches(m.nf);
        }
        const bool last = passes == max_passes;
        const unsigned long long* c;
        if ((rc = pass_front(e, s, m, b, thr2, 0, !last, &launches, &c))) return rc;
        after.read(c);
        if (first) {
            before = after;
            double six;
            std::memcpy(&six, &c[kVolume], 8);
            report->volume_before = six / 6.0;
        }
        if (last) break;
        const int64_t n_new = (int64_t)c[kNewVerts], n_child = (int64_t)c[kChildren];
        const int64_t by[3] = {(int64_t)c[kOne], (int64_t)c[kTwo], (int64_t)c[kThree]};
        if (n_new != (int64_t)c[kMarked] || n_new < 0 || n_new > 3 * m.nf || n_child != m.nf + by[0] + 2 * by[1] + 3 * by[2])
            return set_error(MM_ERR_HIP, "mm_mesh_refine: the scan and the marks disagree");
        if (n_new > 0 && m.nv + n_new > max_vertices) {
            report->stopped_by_cap = 1;
            break;
        }
        report->splits_per_pass[std::min<int64_t>(passes, MM_REFINE_SPLIT_SLOTS - 1)] += n_new;
        ++passes;
        report->faces_by_template[0] += m.nf - by[0] - by[1] - by[2];
        for (int k = 0; k < 3; ++k) report->faces_by_template[k + 1] += by[k];
        if (n_new == 0) {
            report->converged = 1;
            break;
        }
        const Block next{m.nv + n_new, n_child, nv};
        if (next.nv > kMaxIndex || 6 * next.nf > kMaxIndex) return set_error(MM_ERR_TOO_LARGE, "mm_mesh_refine: a pass's result passes 2^31");
        if ((rc = e->ensure(*oth, next.bytes(), false))) return rc;
        unsigned char* to = (unsigned char*)oth->p;
        MM_TRY_HIP(hipMemcpyAsync(to, b, m.o_par(), hipMemcpyDeviceToDevice, e->stream));
        if (m.nv > nv)
            MM_TRY_HIP(hipMemcpyAsync(to + next.o_par(), b + m.o_par(), (size_t)(m.nv - nv) * 8, hipMemcpyDeviceToDevice, e->stream));
        MM_TRY_HIP(launch_refine_offsets(s.code, m.nf, s.tile, s.slot, s.t.keys, s.t.own, (const double*)b, m.nv, nv, s.foff,
                                         (double*)to, (int32_t*)(to + next.o_par()), e->stream));
        MM_TRY_HIP(launch_refine_children((const int32_t*)(b + m.o_face()), m.nf, s.code, s.foff, s.slot, s.t.own,
                                          (const double*)to, (int32_t*)(to + next.o_face()), e->stream));
        launches += 2;
        std::swap(cur, oth);
        m = next;
    }

    // the scratch is that of the last front, which ran over the result
    unsigned char* b = (unsigned char*)cur->p;
    MM_TRY_HIP(launch_weld_volume((const double*)b, (const int32_t*)(b + m.o_face()), m.nf, s.sa, s.sb,
                                  (double*)(s.counts + kVolume), e->stream));
    launches += weld_volume_launches(m.nf);
    const bool fits = vert_cap >= m.nv && face_cap >= m.nf;
    const size_t h_vol = up256(m.bytes());
    if ((rc = e->ensure(e->host_pts, h_vol + 512, true))) return rc;
    unsigned char* hb = (unsigned char*)e->host_pts.p;
    if (fits) MM_TRY_HIP(hipMemcpyAsync(hb, b, m.bytes(), hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(hb + h_vol, s.counts + kVolume, 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    double six;
    std::memcpy(&six, hb + h_vol, 8);
    report->volume_after = six / 6.0;
    report->n_vertices = m.nv;
    report->n_faces = m.nf;
    report->passes_run = passes;
    report->n_edges_before = before.edges; report->n_edges_after = after.edges;
    report->n_open_edges_before = before.open; report->n_open_edges_after = after.open;
    report->n_nonmanifold_edges_before = before.nonmanifold; report->n_nonmanifold_edges_after = after.nonmanifold;
    report->longest_sq_before = before.longest_sq; report->longest_sq_after = after.longest_sq;
    report->n_launches = launches;
    if (!fits) return set_error(MM_ERR_TOO_LARGE, "mm_mesh_refine: vert_cap / face_cap too small (the report holds the sizes)");
    report->bytes_downloaded = (int64_t)m.bytes();
    std::memcpy(out_vertices, hb, (size_t)m.nv * 24);
    widen_faces(out_parents, (const int32_t*)(hb + m.o_par()), 2 * (m.nv - nv));
    widen_faces(out_tris, (const int32_t*)(hb + m.o_face()), 3 * m.nf);
    return MM_OK;
}

}  // extern "C"
