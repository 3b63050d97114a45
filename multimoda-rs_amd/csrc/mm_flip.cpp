// mm_flip.cpp -- CCTA mesh edge flips (include/mm_ccta.h, "mesh edge flips"): the swap of the isotropic remesh, and the
// valences that choose it.  Reference: multimodars/ccta/fixing_functions.py:207-219 (swapflag of MeshLab's filter).  The
// host checks the arguments, narrows the triangles to int32, uploads once, reads one block of counters a pass to decide
// whether another runs, and fills the report; everything over the mesh runs on the device (mm_flip_kernels.hip, the
// volume of mm_weld_kernels.hip).
//
// The mesh, [vertices | faces | mask], lives in e->dev_pts and its faces are rewritten there in place.  What a pass needs
// beside it (the edge table with the first corners, the priorities, the opposite corners, the vertex words, best, the
// counters, the volume's scratch) is carved from e->dev_raw.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/mm_ccta.h"
#include "mm_mesh_layout.h"

namespace mm {
namespace {

int valences(Engine* e, const FlipScratch& s, const int32_t* face, int64_t nf, int64_t nv, const uint8_t* pin, int64_t* launches)
{
    MM_TRY_HIP(launch_flip_valence(face, nf, nv, pin, s.t.keys, s.t.cnt, s.t.own, s.first, s.t.log2_e, s.vw, s.counts,
                                   e->stream));
    *launches += 3;
    return MM_OK;
}

}  // namespace
}  // namespace mm

using namespace mm;

extern "C" {

int mm_mesh_valence(mm_engine* h, const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf,
                    int32_t* out_degree, uint8_t* out_border, int64_t* info)
{
    (void)vertices_xyz;                                                // the valences are the faces' alone
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (!info || (nv > 0 && (!out_degree || !out_border))) return set_error(MM_ERR_INVALID, "mm_mesh_valence: bad arguments");
    if ((rc = mesh_args("mm_mesh_valence", nullptr, nv, tris, nf, false))) return rc;
    std::memset(info, 0, 6 * sizeof(int64_t));
    if (nv == 0 || nf == 0) {                                          // no edge: every vertex has deg 0 and target 6
        for (int64_t v = 0; v < nv; ++v) { out_degree[v] = 0; out_border[v] = 0; }
        info[4] = 36 * nv;
        return MM_OK;
    }
    const size_t fbytes = (size_t)nf * 12;
    if ((rc = e->ensure(e->host_pts, std::max(fbytes, (size_t)nv * 4) + 512, true))) return rc;
    if ((rc = e->ensure(e->dev_pts, fbytes, false))) return rc;
    narrow_faces((int32_t*)e->host_pts.p, tris, 3 * nf);
    MM_TRY_HIP(hipMemcpyAsync(e->dev_pts.p, e->host_pts.p, fbytes, hipMemcpyHostToDevice, e->stream));
    FlipScratch s;
    if ((rc = carve_on(e, e->dev_raw, [&](Carve& c) { s.lay(c, nv, nf); }))) return rc;
    int64_t launches = 0;
    if ((rc = valences(e, s, (const int32_t*)e->dev_pts.p, nf, nv, nullptr, &launches))) return rc;
    unsigned long long c[flip_num_words];
    const unsigned long long* w;
    if ((rc = read_words(e, s.counts, flip_num_words, &w))) return rc;
    std::memcpy(c, w, sizeof(c));
    MM_TRY_HIP(hipMemcpyAsync(e->host_pts.p, s.vw, (size_t)nv * 4, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    const unsigned int* vw = (const unsigned int*)e->host_pts.p;
    for (int64_t v = 0; v < nv; ++v) {
        out_degree[v] = (int32_t)(vw[v] & 0x7FFFFFFFu);
        out_border[v] = (uint8_t)(vw[v] >> 31);
    }
    info[0] = (int64_t)c[flip_num_edges]; info[1] = (int64_t)c[flip_num_open]; info[2] = (int64_t)c[flip_num_nonmanifold];
    info[3] = (int64_t)c[flip_num_inconsistent]; info[4] = (int64_t)c[flip_num_deviation]; info[5] = launches;
    return MM_OK;
}

int mm_mesh_flip_edges(mm_engine* h, const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf,
                       const uint8_t* mask, double crease_cos, double quality_keep, int64_t max_passes, int64_t* out_tris,
                       mm_flip_report* report)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (!report || max_passes < 0 || !(crease_cos >= 0.0 && crease_cos <= 1.0) || !(quality_keep >= 0.0 && quality_keep <= 1.0) ||
        (nf > 0 && !out_tris))
        return set_error(MM_ERR_INVALID, "mm_mesh_flip_edges: bad arguments");
    if ((rc = mesh_args("mm_mesh_flip_edges", vertices_xyz, nv, tris, nf, true))) return rc;
    mm_flip_report rep;
    std::memset(&rep, 0, sizeof(rep));
    rep.n_vertices = nv;
    rep.n_faces = nf;
    if (nv == 0 || nf == 0) {                                          // no edge: nothing to flip, every target is 6
        rep.deviation_before = rep.deviation_after = 36 * nv;
        if (nf > 0 && out_tris != tris) std::memmove(out_tris, tris, (size_t)nf * 24);
        *report = rep;
        return MM_OK;
    }

    const size_t fbytes = (size_t)nf * 12, h_num = up256(fbytes);
    MeshUp up;
    if ((rc = mesh_upload(e, vertices_xyz, nv, tris, nf, mask, h_num + flip_num_words * 8, up))) return rc;
    unsigned char* hb = (unsigned char*)e->host_pts.p;
    const double* v = up.v;
    int32_t* face = up.face;
    const uint8_t* pin = up.pin;

    FlipScratch s;
    if ((rc = carve_on(e, e->dev_raw, [&](Carve& c) { s.lay(c, nv, nf); }))) return rc;
    const double cc2 = crease_cos * crease_cos, qk2 = quality_keep * quality_keep;
    int64_t launches = 0;
    MM_TRY_HIP(launch_weld_volume(v, face, nf, s.sa, s.sb, (double*)(s.counts + flip_num_vol_before), e->stream));
    launches += weld_volume_launches(nf);

    auto edge_counts = [&](const unsigned long long* c) {
        rep.n_edges = (int64_t)c[flip_num_edges]; rep.n_open_edges = (int64_t)c[flip_num_open];
        rep.n_nonmanifold_edges = (int64_t)c[flip_num_nonmanifold];
        rep.n_inconsistent_edges = (int64_t)c[flip_num_inconsistent]; rep.n_masked_edges = (int64_t)c[flip_num_masked];
        rep.deviation_before = (int64_t)c[flip_num_deviation];
    };
    const unsigned long long* c;
    while (rep.passes_run < max_passes) {
        if ((rc = valences(e, s, face, nf, nv, pin, &launches))) return rc;
        MM_TRY_HIP(launch_flip_pass(face, nv, v, pin, s.t.keys, s.t.cnt, s.t.own, s.first, s.t.log2_e, s.vw, cc2, qk2, s.prio,
                                    s.opp, s.best, s.counts, e->stream));
        launches += 2;
        if ((rc = read_words(e, s.counts, flip_num_words, &c))) return rc;
        const int64_t n_cand = (int64_t)c[flip_num_candidates], n_flip = (int64_t)c[flip_num_flips];
        if (n_flip > n_cand || (n_cand > 0 && n_flip == 0))
            return set_error(MM_ERR_HIP, "mm_mesh_flip_edges: the candidates and the flips disagree");
        if (rep.passes_run == 0) edge_counts(c);
        const int64_t slot = std::min<int64_t>(rep.passes_run, MM_FLIP_PASS_SLOTS - 1);
        ++rep.passes_run;
        rep.candidates_per_pass[slot] += n_cand;
        rep.flips_per_pass[slot] += n_flip;
        rep.n_flips += n_flip;
        rep.blocked_existing += (int64_t)c[flip_num_existing]; rep.blocked_normal += (int64_t)c[flip_num_normal];
        rep.blocked_crease += (int64_t)c[flip_num_crease]; rep.blocked_quality += (int64_t)c[flip_num_quality];
        if (n_cand == 0) {                                             // nothing flipped: this pass measured the result
            rep.converged = 1;
            rep.deviation_after = (int64_t)c[flip_num_deviation];
            break;
        }
    }
    if (!rep.converged) {                                              // the valences of the result, a pass of their own
        if ((rc = valences(e, s, face, nf, nv, pin, &launches))) return rc;
        if ((rc = read_words(e, s.counts, flip_num_words, &c))) return rc;
        if (rep.passes_run == 0) edge_counts(c);
        rep.deviation_after = (int64_t)c[flip_num_deviation];
    }

    MM_TRY_HIP(launch_weld_volume(v, face, nf, s.sa, s.sb, (double*)(s.counts + flip_num_vol_after), e->stream));
    launches += weld_volume_launches(nf);
    MM_TRY_HIP(hipMemcpyAsync(hb, face, fbytes, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(hb + h_num, s.counts, flip_num_words * 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    double six[2];
    std::memcpy(six, hb + h_num + flip_num_vol_before * 8, 16);
    rep.volume_before = six[0] / 6.0;
    rep.volume_after = six[1] / 6.0;
    rep.n_launches = launches;
    rep.bytes_uploaded = (int64_t)up.up_bytes;
    rep.bytes_downloaded = (int64_t)(fbytes + flip_num_words * 8);
    widen_faces(out_tris, (const int32_t*)hb, 3 * nf);
    *report = rep;
    return MM_OK;
}

}  // extern "C"
