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
#include "mm_stage.h"

namespace mm {
namespace {

struct Scratch {
    EdgeTable t;
    size_t o_rep, o_wf, o_qb, o_frep, o_fkeep, o_table, o_eslot, o_m1q, o_m2q, o_m1f, o_m2f, o_link, o_changed, o_vmin,
        o_ref, o_vsplit, o_vkeep, o_isnew, o_wmin, o_wmax, o_vback, o_mixed, o_cback, o_vtile, o_ftile, o_ctile, o_vidx, o_fidx, o_cidx, o_counts, o_out_v, o_out_f,
        o_origin, o_target, size;
    int log2_v, log2_f;
    int32_t *rep, *wf, *frep, *table, *m1f, *m2f, *vidx, *fidx, *cidx, *out_f, *origin, *target;
    unsigned long long *qb, *m1q, *m2q, *counts;
    unsigned int *eslot, *link, *changed, *vmin, *wmin, *wmax;
    uint8_t *fkeep, *ref, *vsplit, *vkeep, *isnew, *vback, *mixed, *cback;
    long long *vtile, *ftile, *ctile;
    double* out_v;

    void plan(int64_t nv, int64_t nf)
    {
        Carve lay;
        t.plan(lay, nf);
        const size_t cap = (size_t)1 << t.log2_e, V = (size_t)nv, Fn = (size_t)nf, Cn = 3 * Fn;
        log2_v = log2_at_least(2ull * V); log2_f = log2_at_least(2ull * Fn);
        o_rep = lay.take(V * 4); o_wf = lay.take(Cn * 4); o_qb = lay.take(Fn * 8); o_frep = lay.take(Fn * 4);
        o_fkeep = lay.take(Fn); o_table = lay.take(((size_t)1 << std::max(log2_v, log2_f)) * 4);
        o_eslot = lay.take(Cn * 4); o_m1q = lay.take(cap * 8); o_m2q = lay.take(cap * 8); o_m1f = lay.take(cap * 4);
        o_m2f = lay.take(cap * 4); o_link = lay.take(Cn * 4); o_changed = lay.take(4);
        o_vmin = lay.take(V * 4); o_ref = lay.take(V); o_vsplit = lay.take(V); o_vkeep = lay.take(V); o_isnew = lay.take(Cn);
        o_wmin = lay.take(V * 4); o_wmax = lay.take(V * 4); o_vback = lay.take(V); o_mixed = lay.take(Cn); o_cback = lay.take(Cn);
        o_vtile = lay.take((trim_scan_tiles(nv) + 1) * 8); o_ftile = lay.take((trim_scan_tiles(nf) + 1) * 8);
        o_ctile = lay.take((trim_scan_tiles(3 * nf) + 1) * 8);
        o_vidx = lay.take(V * 4); o_fidx = lay.take(Fn * 4); o_cidx = lay.take(Cn * 4);
        o_counts = lay.take(rep_num_words * 8);
        o_out_v = lay.take((V + Cn) * 24); o_out_f = lay.take(Cn * 4); o_origin = lay.take((V + Cn) * 4);
        o_target = lay.take(V * 4);
        size = lay.size();
    }
    void bind(unsigned char* b)
    {
        t.bind(b);
        rep = (int32_t*)(b + o_rep); wf = (int32_t*)(b + o_wf); qb = (unsigned long long*)(b + o_qb);
        frep = (int32_t*)(b + o_frep); fkeep = b + o_fkeep; table = (int32_t*)(b + o_table);
        eslot = (unsigned int*)(b + o_eslot); m1q = (unsigned long long*)(b + o_m1q); m2q = (unsigned long long*)(b + o_m2q);
        m1f = (int32_t*)(b + o_m1f); m2f = (int32_t*)(b + o_m2f); link = (unsigned int*)(b + o_link);
        changed = (unsigned int*)(b + o_changed); vmin = (unsigned int*)(b + o_vmin);
        ref = b + o_ref; vsplit = b + o_vsplit; vkeep = b + o_vkeep; isnew = b + o_isnew;
        wmin = (unsigned int*)(b + o_wmin); wmax = (unsigned int*)(b + o_wmax); vback = b + o_vback; mixed = b + o_mixed;
        cback = b + o_cback;
        vtile = (long long*)(b + o_vtile); ftile = (long long*)(b + o_ftile); ctile = (long long*)(b + o_ctile);
        vidx = (int32_t*)(b + o_vidx); fidx = (int32_t*)(b + o_fidx); cidx = (int32_t*)(b + o_cidx);
        counts = (unsigned long long*)(b + o_counts);
        out_v = (double*)(b + o_out_v); out_f = (int32_t*)(b + o_out_f); origin = (int32_t*)(b + o_origin);
        target = (int32_t*)(b + o_target);
    }
};

}  // namespace
}  // namespace mm

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
    if (!report || nv < 0 || nf < 0 || vert_cap < 0 || nv > kMaxIndex || nf > kMaxIndex || (flags & ~MM_REPAIR_ALL_FLAGS) ||
        (nv > 0 && (!vertices_xyz || !out_target)) || (vert_cap > 0 && (!out_vertices || !out_origin)) ||
        (nf > 0 && (!faces || !out_faces)))
        return set_error(MM_ERR_INVALID, std::string(who) + ": bad arguments");
    for (int64_t k = 0; k < 3 * nv; ++k)
        if (!std::isfinite(vertices_xyz[k])) return set_error(MM_ERR_INVALID, std::string(who) + ": non-finite coordinate");
    if ((rc = faces_in_range(faces, nf, nv, who))) return rc;
    if (6 * nf > kMaxIndex) return set_error(MM_ERR_TOO_LARGE, std::string(who) + ": 6 nf passes 2^31");
    mm_repair_report rep;
    std::memset(&rep, 0, sizeof(rep));
    if (nv == 0) {                                                     // no vertex, so no face either
        *report = rep;
        return MM_OK;
    }

    const size_t vbytes = (size_t)nv * 24, fbytes = (size_t)nf * 12, up_bytes = vbytes + fbytes;
    Scratch s;
    s.plan(nv, nf);
    // the host side of the download, worst case: every corner a new vertex
    const size_t most_v = (size_t)nv + 3 * (size_t)nf;
    const size_t h_f = up256(most_v * 24), h_origin = h_f + up256(fbytes), h_target = h_origin + up256(most_v * 4);
    const size_t h_num = h_target + up256((size_t)nv * 4), h_end = h_num + rep_num_words * 8 + 3 * 8;
    if ((rc = e->ensure(e->host_pts, std::max(up_bytes, h_end) + 512, true))) return rc;
    if ((rc = e->ensure(e->dev_pts, up_bytes, false))) return rc;
    if ((rc = e->ensure(e->dev_raw, s.size, false))) return rc;
    unsigned char* hb = (unsigned char*)e->host_pts.p;
    unsigned char* b = (unsigned char*)e->dev_pts.p;
    s.bind((unsigned char*)e->dev_raw.p);
    std::memcpy(hb, vertices_xyz, vbytes);
    narrow_faces((int32_t*)(hb + vbytes), faces, 3 * nf);
    MM_TRY_HIP(hipMemcpyAsync(b, hb, up_bytes, hipMemcpyHostToDevice, e->stream));
    const double* v = (const double*)b;
    const int32_t* face = (const int32_t*)(b + vbytes);

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
    rep.bytes_uploaded = (int64_t)up_bytes;
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
