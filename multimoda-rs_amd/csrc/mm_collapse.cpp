// mm_collapse.cpp -- CCTA mesh edge collapse (include/mm_ccta.h, "mesh edge collapse"): the collapse of the isotropic
// remesh.  Reference: multimodars/ccta/fixing_functions.py:207-219 (collapseflag of MeshLab's filter).  The host checks the
// arguments, narrows the triangles to int32, uploads once, reads one block of counters a pass to decide whether another
// runs, and fills the report; everything over the mesh runs on the device (mm_collapse_kernels.hip, the adjacency of
// mm_smooth_kernels.hip, the scan and the compaction of mm_trim_kernels.hip, the volume of mm_weld_kernels.hip).
//
// The mesh, [vertices | faces | mask], lives in e->dev_pts: the vertices are never written, the faces are rewritten where
// they lie.  What a pass needs beside it is carved from e->dev_raw: the edge table with the first corners, and apart from
// its owner words the adjacency rows (CsrDev of mm_stage.h lays them over the owners; the collapse reads both), the
// priorities, the two ends, the vertex words, best, the liveness bytes, the links r -> k, the counters; then what the end
// needs: the scans, the compacted mesh, origin and target, the volume's scratch.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/mm_ccta.h"
#include "mm_mesh_layout.h"

using namespace mm;

extern "C" {

int mm_mesh_collapse_edges(mm_engine* h, const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf,
                           const uint8_t* mask, double target_len, double min_ratio, double max_ratio, double crease_cos,
                           double quality_keep, int64_t max_passes, double* out_vertices, int64_t* out_tris,
                           int64_t* out_origin, int64_t* out_target, mm_collapse_report* report)
{
    static const char* who = "mm_mesh_collapse_edges";
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (!report || max_passes < 0 || !(crease_cos >= 0.0 && crease_cos <= 1.0) || !(quality_keep >= 0.0 && quality_keep <= 1.0) ||
        !(target_len > 0.0) || !std::isfinite(target_len) || !(min_ratio > 0.0 && min_ratio <= 1.0) ||
        !(max_ratio >= 1.0) || !std::isfinite(max_ratio) || (nv > 0 && (!out_vertices || !out_origin || !out_target)) ||
        (nf > 0 && !out_tris))
        return set_error(MM_ERR_INVALID, std::string(who) + ": bad arguments");
    if ((rc = mesh_args(who, vertices_xyz, nv, tris, nf, true))) return rc;
    mm_collapse_report rep;
    std::memset(&rep, 0, sizeof(rep));
    rep.n_vertices = rep.n_vertices_out = nv;
    rep.n_faces = rep.n_faces_out = nf;
    if (nv == 0 || nf == 0) {                                          // no edge: nothing to collapse
        if (nv > 0 && out_vertices != vertices_xyz) std::memmove(out_vertices, vertices_xyz, (size_t)nv * 24);
        if (nf > 0 && out_tris != tris) std::memmove(out_tris, tris, (size_t)nf * 24);
        for (int64_t v = 0; v < nv; ++v) out_origin[v] = out_target[v] = v;
        *report = rep;
        return MM_OK;
    }

    const size_t vbytes = (size_t)nv * 24, fbytes = (size_t)nf * 12;
    const size_t h_f = up256(vbytes), h_origin = h_f + up256(fbytes), h_target = h_origin + up256((size_t)nv * 4);
    const size_t h_num = h_target + up256((size_t)nv * 4);
    MeshUp up;
    if ((rc = mesh_upload(e, vertices_xyz, nv, tris, nf, mask, h_num + col_num_words * 8, up))) return rc;
    unsigned char* hb = (unsigned char*)e->host_pts.p;
    const double* v = up.v;
    int32_t* face = up.face;
    const uint8_t* pin = up.pin;

    CollapseScratch s;
    if ((rc = carve_on(e, e->dev_raw, [&](Carve& c) { s.lay(c, nv, nf); }))) return rc;
    const double lo_len = min_ratio * target_len, hi_len = max_ratio * target_len;
    const double thr_min2 = lo_len * lo_len, thr_max2 = hi_len * hi_len;
    const double cc2 = crease_cos * crease_cos, qk2 = quality_keep * quality_keep;
    int64_t launches = 0;
    MM_TRY_HIP(hipMemsetAsync(s.fkeep, 1, (size_t)nf, e->stream));
    MM_TRY_HIP(hipMemsetAsync(s.vkeep, 1, (size_t)nv, e->stream));
    MM_TRY_HIP(hipMemsetAsync(s.to, 0xFF, (size_t)nv * 4, e->stream));
    MM_TRY_HIP(hipMemsetAsync(s.counts, 0, col_num_words * 8, e->stream));
    MM_TRY_HIP(launch_weld_volume(v, face, nf, s.sa, s.sb, (double*)(s.counts + col_num_vol_before), e->stream));
    launches += weld_volume_launches(nf);

    auto table = [&]() -> int {
        MM_TRY_HIP(launch_col_table(face, nf, s.fkeep, nv, v, thr_min2, s.t.keys, s.t.cnt, s.t.own, s.first, s.t.log2_e, s.vw,
                                    s.prio, s.counts, e->stream));
        launches += 2;
        return MM_OK;
    };
    auto edge_counts = [&](const unsigned long long* c) {
        rep.n_edges = (int64_t)c[col_num_edges]; rep.n_open_edges = (int64_t)c[col_num_open];
        rep.n_nonmanifold_edges = (int64_t)c[col_num_nonmanifold];
        rep.n_inconsistent_edges = (int64_t)c[col_num_inconsistent]; rep.n_short_before = (int64_t)c[col_num_short];
    };
    const unsigned long long* c;
    while (rep.passes_run < max_passes) {
        if ((rc = table())) return rc;
        int csr_launches = 0;
        MM_TRY_HIP(launch_mesh_csr(s.t.keys, s.t.log2_e, nv, s.deg, s.off, s.tile, s.nb, s.csr_counts, &csr_launches, e->stream));
        launches += csr_launches;
        MM_TRY_HIP(launch_col_pass(face, nv, v, pin, s.t.keys, s.t.own, s.first, s.t.log2_e, s.vw, s.off, s.nb,
                                   thr_max2, cc2, qk2, s.prio, s.rk, s.best, s.fkeep, s.vkeep, s.to, s.counts,
                                   e->stream));
        launches += 2;
        if ((rc = read_words(e, s.counts, col_num_words, &c))) return rc;
        const int64_t n_cand = (int64_t)c[col_num_candidates], n_col = (int64_t)c[col_num_collapses];
        if (n_col > n_cand || (n_cand > 0 && n_col == 0))
            return set_error(MM_ERR_HIP, std::string(who) + ": the candidates and the collapses disagree");
        if (rep.passes_run == 0) edge_counts(c);
        const int64_t slot = std::min<int64_t>(rep.passes_run, MM_COLLAPSE_PASS_SLOTS - 1);
        ++rep.passes_run;
        rep.candidates_per_pass[slot] += n_cand;
        rep.collapses_per_pass[slot] += n_col;
        rep.n_collapses += n_col;
        rep.blocked_fixed += (int64_t)c[col_num_fixed]; rep.blocked_link += (int64_t)c[col_num_link];
        rep.blocked_valence += (int64_t)c[col_num_valence]; rep.blocked_long += (int64_t)c[col_num_long];
        rep.blocked_normal += (int64_t)c[col_num_normal]; rep.blocked_quality += (int64_t)c[col_num_quality];
        if (n_cand == 0) {                                             // nothing collapsed: this pass measured the result
            rep.converged = 1;
            rep.n_short_after = (int64_t)c[col_num_short];
            break;
        }
    }
    if (!rep.converged) {                                              // the short edges of the result, a table of their own
        if ((rc = table())) return rc;
        if ((rc = read_words(e, s.counts, col_num_words, &c))) return rc;
        if (rep.passes_run == 0) edge_counts(c);
        rep.n_short_after = (int64_t)c[col_num_short];
    }

    // one stable compaction: the trim's scans over the liveness bytes, its gather and remap; then origin and target
    MM_TRY_HIP(launch_trim_scan(s.vkeep, nv, s.vtile, s.vidx, e->stream));
    MM_TRY_HIP(launch_trim_scan(s.fkeep, nf, s.ftile, s.fidx, e->stream));
    MM_TRY_HIP(launch_trim_compact(v, nv, s.vidx, face, nf, s.fidx, s.out_v, s.out_f, e->stream));
    MM_TRY_HIP(launch_col_finish(s.to, s.vidx, nv, s.origin, s.target, e->stream));
    launches += 9;
    long long kv = 0, kf = 0;
    if ((rc = scan_totals(e, s.vtile, nv, s.ftile, nf, &kv, &kf, who))) return rc;
    if (nv - kv != rep.n_collapses || nf - kf != 2 * rep.n_collapses)
        return set_error(MM_ERR_HIP, std::string(who) + ": the compaction and the collapses disagree");
    if (kf > 0) {
        MM_TRY_HIP(launch_weld_volume(s.out_v, s.out_f, kf, s.sa, s.sb, (double*)(s.counts + col_num_vol_after), e->stream));
        launches += weld_volume_launches(kf);
    }
    MM_TRY_HIP(hipMemcpyAsync(hb, s.out_v, (size_t)kv * 24, hipMemcpyDeviceToHost, e->stream));
    if (kf > 0) MM_TRY_HIP(hipMemcpyAsync(hb + h_f, s.out_f, (size_t)kf * 12, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(hb + h_origin, s.origin, (size_t)kv * 4, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(hb + h_target, s.target, (size_t)nv * 4, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(hb + h_num, s.counts, col_num_words * 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    double six[2];
    std::memcpy(six, hb + h_num + col_num_vol_before * 8, 16);
    rep.volume_before = six[0] / 6.0;
    rep.volume_after = six[1] / 6.0;
    rep.n_vertices_out = kv;
    rep.n_faces_out = kf;
    rep.n_launches = launches;
    rep.bytes_uploaded = (int64_t)up.up_bytes;
    rep.bytes_downloaded = (int64_t)((size_t)kv * 28 + (size_t)kf * 12 + (size_t)nv * 4 + col_num_words * 8);
    std::memcpy(out_vertices, hb, (size_t)kv * 24);
    widen_faces(out_tris, (const int32_t*)(hb + h_f), 3 * kf);
    const int32_t *ho = (const int32_t*)(hb + h_origin), *ht = (const int32_t*)(hb + h_target);
    for (int64_t i = 0; i < kv; ++i) out_origin[i] = ho[i];
    for (int64_t i = 0; i < nv; ++i) out_target[i] = ht[i];
    *report = rep;
    return MM_OK;
}

}  // extern "C"
