// mm_repair.cpp -- CCTA mesh repair (include/mm_ccta.h, "mesh repair"): duplicate vertices, degenerate, null and duplicate
// faces, non-manifold edges and vertices, unreferenced vertices.  Reference: multimodars/ccta/fixing_functions.py:114-239
// (MeshLab's five repair filters).  The host checks the arguments, narrows the faces to int32, uploads once, reads one
// word a pointer-jumping round and the counters with the three scan totals before the output is written, and fills the
// report; everything over the mesh runs on the device (mm_repair_kernels.hip, the edge report and the jumping round of
// mm_weld_kernels.hip, the scan of mm_trim_kernels.hip).
//
// The mesh, [vertices | faces], lives in e->dev_pts and is never written.  The rest is carved from e->dev_raw: the names
// (rep), the faces through them (wf), q, the face slots, the liveness bytes, one int32 table for vertices and then faces,
// the edge table with the corner slots and the four planes of the two largest keys, the corner links, the planes of the
// split, the three scans, and the output: the vertices kept and the new ones (at most one a corner), faces, origin, target.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/mm_ccta.h"
#include "mm_mesh_layout.h"

using namespace mm;

extern "C" {

int mm_mesh_repair(mm_engine* h, const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf, int flags,
                   int64_t vert_cap, double* out_vertices, int64_t* out_faces, int64_t* out_origin, int64_t* out_target,
                   mm_repair_report* report)
{
    static const char* who = "mm_mesh_repair";
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (!report || vert_cap < 0 || (flags & ~MM_REPAIR_ALL_FLAGS) || (nv > 0 && !out_target) ||
        (vert_cap > 0 && (!out_vertices || !out_origin)) || (nf > 0 && !out_faces))
        return set_error(MM_ERR_INVALID, std::string(who) + ": bad arguments");
    if ((rc = mesh_args(who, vertices_xyz, nv, faces, nf, true))) return rc;
    for (int64_t k = 0; k < 3 * nv; ++k)
        if (!std::isfinite(vertices_xyz[k])) return set_error(MM_ERR_INVALID, std::string(who) + ": non-finite coordinate");
    mm_repair_report rep;
    std::memset(&rep, 0, sizeof(rep));
    if (nv == 0) {                                                     // no vertex, so no face either
        *report = rep;
        return MM_OK;
    }

    // the host side of the download, worst case: every corner a new vertex
    const size_t fbytes = (size_t)nf * 12, most_v = (size_t)nv + 3 * (size_t)nf;
    const size_t h_f = up256(most_v * 24), h_origin = h_f + up256(fbytes), h_target = h_origin + up256(most_v * 4);
    const size_t h_num = h_target + up256((size_t)nv * 4), h_end = h_num + rep_num_words * 8 + 3 * 8;
    MeshUp up;
    if ((rc = mesh_upload(e, vertices_xyz, nv, faces, nf, nullptr, h_end, up))) return rc;
    RepairScratch s;
    if ((rc = carve_on(e, e->dev_raw, [&](Carve& c) { s.lay(c, nv, nf); }))) return rc;
    unsigned char* hb = (unsigned char*)e->host_pts.p;
    const double* v = up.v;
    const int32_t* face = up.face;

    int64_t launches = 0;
    MM_TRY_HIP(hipMemsetAsync(s.counts, 0, rep_num_words * 8, e->stream));
    MM_TRY_HIP(launch_rep_vertices(v, nv, flags & MM_REPAIR_DUPLICATE_VERTICES, s.table, s.log2_v, s.rep, s.counts, e->stream));
    MM_TRY_HIP(launch_rep_faces(face, nf, s.rep, v, flags & MM_REPAIR_NULL_FACES, flags & MM_REPAIR_DUPLICATE_FACES, s.table,
                                s.log2_f, s.wf, s.qb, s.frep, s.fkeep, s.counts, e->stream));
    MM_TRY_HIP(launch_rep_edges(s.wf, nf, s.fkeep, s.t.keys, s.t.cnt, s.t.own, s.t.log2_e, s.eslot, e->stream));
    MM_TRY_HIP(launch_weld_edge_report(s.t.keys, s.t.cnt, s.t.own, s.t.log2_e, nullptr, s.counts + rep_num_edges_before,
                                       e->stream));
    MM_TRY_HIP(launch_rep_remove(nf, s.fkeep, s.eslot, s.t.cnt, s.qb, s.t.log2_e, flags & MM_REPAIR_NONMANIFOLD_EDGES, s.m1q,
                                 s.m1f, s.m2q, s.m2f, s.link, s.counts, e->stream));
    MM_TRY_HIP(launch_rep_edges(s.wf, nf, s.fkeep, s.t.keys, s.t.cnt, s.t.own, s.t.log2_e, s.eslot, e->stream));
    MM_TRY_HIP(launch_weld_edge_report(s.t.keys, s.t.cnt, s.t.own, s.t.log2_e, nullptr, s.counts + rep_num_edges_after,
                                       e->stream));
    MM_TRY_HIP(launch_rep_hook(s.t.keys, s.t.cnt, s.t.own, s.t.log2_e, s.wf, s.link, e->stream));
    launches += 2 + 2 + 2 + 5 + 2 + 1;
    if (nf > 0) {                                                      // flatten the links: rounds until one moves nothing
        unsigned int* hc = (unsigned int*)hb;
        const int64_t bound = 2 + log2_at_least(3ull * (unsigned long long)nf) + 8;   // never reached: see the header
        for (;;) {
            MM_TRY_HIP(launch_weld_jump(s.link, 3 * nf, s.changed, e->stream));
            MM_TRY_HIP(hipMemcpyAsync(hc, s.changed, 4, hipMemcpyDeviceToHost, e->stream));
            MM_TRY_HIP(hipStreamSynchronize(e->stream));
            ++rep.union_rounds;
            if (!hc[0]) break;
            if (rep.union_rounds > bound) return set_error(MM_ERR_HIP, std::string(who) + ": pointer jumping did not settle");
        }
    }
    MM_TRY_HIP(launch_rep_split(nf, nv, s.fkeep, face, s.wf, s.link, s.rep, flags & MM_REPAIR_NONMANIFOLD_VERTICES,
                                flags & MM_REPAIR_DROP_UNREFERENCED, s.vmin, s.wmin, s.wmax, s.ref, s.vsplit, s.vback, s.mixed,
                                s.isnew, s.cback, s.vkeep, s.counts, e->stream));
    MM_TRY_HIP(launch_trim_scan(s.isnew, 3 * nf, s.ctile, s.cidx, e->stream));
    MM_TRY_HIP(launch_trim_scan(s.vkeep, nv, s.vtile, s.vidx, e->stream));
    MM_TRY_HIP(launch_trim_scan(s.fkeep, nf, s.ftile, s.fidx, e->stream));
    launches += 3 + 3 + (nf > 0 ? 6 : 0);

    // the counters and the three totals: what the output holds, and whether it fits
    unsigned long long* hn = (unsigned long long*)(hb + h_num);
    MM_TRY_HIP(hipMemcpyAsync(hn, s.counts, rep_num_words * 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(hn + rep_num_words, s.vtile + trim_scan_tiles(nv), 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(hn + rep_num_words + 1, s.ftile + trim_scan_tiles(nf), 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(hn + rep_num_words + 2, s.ctile + trim_scan_tiles(3 * nf), 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    const int64_t kv = (int64_t)hn[rep_num_words], kf = (int64_t)hn[rep_num_words + 1], kn = (int64_t)hn[rep_num_words + 2];
    if (kv < 0 || kv > nv || kf < 0 || kf > nf || kn < 0 || kn > 3 * nf)
        return set_error(MM_ERR_HIP, std::string(who) + ": compaction count out of range");
    rep.n_vertices = kv + kn;
    rep.n_faces = kf;
    rep.n_welded_vertices = (int64_t)hn[rep_num_welded] - (int64_t)hn[rep_num_unwelded];
    rep.n_degenerate_faces = (int64_t)hn[rep_num_degenerate];
    rep.n_null_faces = (int64_t)hn[rep_num_null];
    rep.n_duplicate_faces = (int64_t)hn[rep_num_copies];
    rep.n_open_edges_before = (int64_t)hn[rep_num_edges_before];
    rep.n_nonmanifold_edges_before = (int64_t)hn[rep_num_edges_before + 1];
    rep.n_open_edges_after = (int64_t)hn[rep_num_edges_after];
    rep.n_nonmanifold_edges_after = (int64_t)hn[rep_num_edges_after + 1];
    rep.n_faces_removed = (int64_t)hn[rep_num_removed];
    rep.n_nonmanifold_vertices = (int64_t)hn[rep_num_split];
    rep.n_new_vertices = kn;
    rep.n_unreferenced_dropped = (int64_t)hn[rep_num_unreferenced];
    rep.bytes_uploaded = (int64_t)up.up_bytes;
    rep.bytes_downloaded = (int64_t)((size_t)rep.n_vertices * 28 + (size_t)kf * 12 + (size_t)nv * 4 + rep_num_words * 8 + 24);
    rep.n_launches = launches + 2 + rep.union_rounds;
    if (rep.n_vertices > kMaxIndex) return set_error(MM_ERR_TOO_LARGE, std::string(who) + ": the result passes 2^31 vertices");
    if (rep.n_vertices > vert_cap) {
        *report = rep;
        return set_error(MM_ERR_TOO_LARGE, std::string(who) + ": vert_cap is too small for the new vertices");
    }

    MM_TRY_HIP(launch_rep_output(v, nv, s.rep, s.vidx, nf, s.fkeep, s.fidx, face, s.wf, s.link, s.cback, s.cidx, kv, s.out_v, s.out_f,
                                 s.origin, s.target, e->stream));
    const size_t nout = (size_t)rep.n_vertices;
    if (nout > 0) {
        MM_TRY_HIP(hipMemcpyAsync(hb, s.out_v, nout * 24, hipMemcpyDeviceToHost, e->stream));
        MM_TRY_HIP(hipMemcpyAsync(hb + h_origin, s.origin, nout * 4, hipMemcpyDeviceToHost, e->stream));
    }
    if (kf > 0) MM_TRY_HIP(hipMemcpyAsync(hb + h_f, s.out_f, (size_t)kf * 12, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(hb + h_target, s.target, (size_t)nv * 4, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    std::memcpy(out_vertices, hb, nout * 24);
    widen_faces(out_faces, (const int32_t*)(hb + h_f), 3 * kf);
    const int32_t *ho = (const int32_t*)(hb + h_origin), *ht = (const int32_t*)(hb + h_target);
    for (size_t i = 0; i < nout; ++i) out_origin[i] = ho[i];
    for (int64_t i = 0; i < nv; ++i) out_target[i] = ht[i];
    *report = rep;
    return MM_OK;
}

}  // extern "C"
