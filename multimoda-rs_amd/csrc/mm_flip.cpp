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
#include "mm_stage.h"

namespace mm {
namespace {

int flip_args(int64_t nv, const int64_t* tris, int64_t nf, const char* who)
{
    if (nv < 0 || nf < 0 || nv > kMaxIndex || nf > kMaxIndex || (nf > 0 && !tris))
        return set_error(MM_ERR_INVALID, std::string(who) + ": bad arguments");
    if (const int rc = faces_in_range(tris, nf, nv, who)) return rc;
    if (6 * nf > kMaxIndex) return set_error(MM_ERR_TOO_LARGE, std::string(who) + ": 6 nf passes 2^31");
    return MM_OK;
}

struct Scratch {
    EdgeTable t;
    size_t o_first, o_prio, o_opp, o_vw, o_best, o_counts, o_sa, o_sb, size;
    unsigned int *first, *vw;
    unsigned long long *prio, *best, *counts;
    int32_t* opp;
    double *sa, *sb;

    void plan(int64_t nv, int64_t nf)
    {
        Carve lay;
        t.plan(lay, nf);
        const size_t cap = (size_t)1 << t.log2_e;
        o_first = lay.take(cap * 4); o_prio = lay.take(cap * 8); o_opp = lay.take(cap * 8);
        o_vw = lay.take((size_t)nv * 4); o_best = lay.take((size_t)nv * 8); o_counts = lay.take(flip_num_words * 8);
        o_sa = lay.take((size_t)nf * 8); o_sb = lay.take(weld_sum_scratch(nf) * 8);
        size = lay.size();
    }
    void bind(unsigned char* b)
    {
        t.bind(b);
        first = (unsigned int*)(b + o_first); prio = (unsigned long long*)(b + o_prio); opp = (int32_t*)(b + o_opp);
        vw = (unsigned int*)(b + o_vw); best = (unsigned long long*)(b + o_best);
        counts = (unsigned long long*)(b + o_counts); sa = (double*)(b + o_sa); sb = (double*)(b + o_sb);
    }
};

// the counters of a pass, or of the valences alone, through the first words of e->host_pts (behind the upload in stream
// order)
int read_counts(Engine* e, const Scratch& s, const unsigned long long** words)
{
    MM_TRY_HIP(hipMemcpyAsync(e->host_pts.p, s.counts, flip_num_words * 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    *words = (const unsigned long long*)e->host_pts.p;
    return MM_OK;
}

int valences(Engine* e, const Scratch& s, const int32_t* face, int64_t nf, int64_t nv, const uint8_t* pin, int64_t* launches)
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
    if ((rc = flip_args(nv, tris, nf, "mm_mesh_valence"))) return rc;
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
    Scratch s;
    s.plan(nv, nf);
    if ((rc = e->ensure(e->dev_raw, s.size, false))) return rc;
    s.bind((unsigned char*)e->dev_raw.p);
    int64_t launches = 0;
    if ((rc = valences(e, s, (const int32_t*)e->dev_pts.p, nf, nv, nullptr, &launches))) return rc;
    unsigned long long c[flip_num_words];
    const unsigned long long* w;
    if ((rc = read_counts(e, s, &w))) return rc;
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
        (nv > 0 && !vertices_xyz) || (nf > 0 && !out_tris))
        return set_error(MM_ERR_INVALID, "mm_mesh_flip_edges: bad arguments");
    if ((rc = flip_args(nv, tris, nf, "mm_mesh_flip_edges"))) return rc;
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

    const size_t vbytes = (size_t)nv * 24, fbytes = (size_t)nf * 12, up_bytes = vbytes + fbytes + (mask ? (size_t)nv : 0);
    const size_t h_num = up256(fbytes);
    if ((rc = e->ensure(e->host_pts, std::max(up_bytes, h_num + flip_num_words * 8) + 512, true))) return rc;
    if ((rc = e->ensure(e->dev_pts, up_bytes, false))) return rc;
    unsigned char* hb = (unsigned char*)e->host_pts.p;
    unsigned char* b = (unsigned char*)e->dev_pts.p;
    std::memcpy(hb, vertices_xyz, vbytes);
    narrow_faces((int32_t*)(hb + vbytes), tris, 3 * nf);
    if (mask) std::memcpy(hb + vbytes + fbytes, mask, (size_t)nv);
    MM_TRY_HIP(hipMemcpyAsync(b, hb, up_bytes, hipMemcpyHostToDevice, e->stream));
    const double* v = (const double*)b;
    int32_t* face = (int32_t*)(b + vbytes);
    const uint8_t* pin = mask ? b + vbytes + fbytes : nullptr;

    Scratch s;
    s.plan(nv, nf);
    if ((rc = e->ensure(e->dev_raw, s.size, false))) return rc;
    s.bind((unsigned char*)e->dev_raw.p);
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
        if ((rc = read_counts(e, s, &c))) return rc;
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
        if ((rc = read_counts(e, s, &c))) return rc;
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
    rep.bytes_uploaded = (int64_t)up_bytes;
    rep.bytes_downloaded = (int64_t)(fbytes + flip_num_words * 8);
    widen_faces(out_tris, (const int32_t*)hb, 3 * nf);
    *report = rep;
    return MM_OK;
}

}  // extern "C"
