// mm_relax.cpp -- CCTA mesh relaxation (include/mm_ccta.h, "mesh relaxation"): tangential smoothing of the free vertices
// of a mesh, every step reprojected onto a reference surface.  Reference: the smoothing and reprojection of MeshLab's
// isotropic remesh as multimodars/ccta/fixing_functions.py:192-219 asks for it (smoothflag, reprojectflag).  The host
// checks the arguments, finds the free vertices (adjacency, mask, border edges), plans step 0 of the point-to-triangle
// search over them (mm_tri_plan.h) and uploads once; every position, distance, bound and count after that is computed
// on the device (mm_tri_kernels.hip, mm_relax_kernels.hip, mm_smooth_kernels.hip, mm_weld_kernels.hip), and one copy
// brings the vertices, the faces the free vertices lie on and the report's numbers back.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/mm_ccta.h"
#include "mm_tri_plan.h"

namespace mm {
namespace {

// flags[v]: bit 0 = v has a neighbour (an edge to a different vertex), bit 1 = v ends an edge whose owner count is not 2
// (every corner pair of every face owns its undirected edge, an (a, a) pair too: as mm_fill_holes counts)
void vertex_flags(const int64_t* f, int64_t nf, int64_t nv, std::vector<uint8_t>& flags)
{
    flags.assign((size_t)nv, 0);
    std::vector<uint64_t> keys((size_t)(3 * nf));
    for (int64_t i = 0; i < nf; ++i)
        for (int k = 0; k < 3; ++k) {
            const uint64_t a = (uint64_t)f[3 * i + k], b = (uint64_t)f[3 * i + (k + 1) % 3];
            keys[(size_t)(3 * i + k)] = (std::min(a, b) << 32) | std::max(a, b);
            if (a != b) { flags[(size_t)a] |= 1; flags[(size_t)b] |= 1; }
        }
    std::sort(keys.begin(), keys.end());
    for (size_t i = 0; i < keys.size();) {
        size_t j = i + 1;
        while (j < keys.size() && keys[j] == keys[i]) ++j;
        if (j - i != 2) { flags[(size_t)(keys[i] >> 32)] |= 2; flags[(size_t)(keys[i] & 0xffffffffull)] |= 2; }
        i = j;
    }
}

}  // namespace
}  // namespace mm

using namespace mm;

extern "C" {

int mm_mesh_relax(mm_engine* h, const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf,
                  const double* ref_vertices, int64_t ref_nv, const int64_t* ref_tris, int64_t ref_nf,
                  const uint8_t* pinned, int64_t n_iterations, double factor, double* out_vertices, int64_t* out_ref_face,
                  mm_relax_report* report)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    const char* who = "mm_mesh_relax";
    if (!report || n_iterations < 0 || !std::isfinite(factor) || (nv > 0 && (!out_vertices || !out_ref_face)))
        return set_error(MM_ERR_INVALID, "mm_mesh_relax: bad arguments");
    if (!ref_vertices) { ref_vertices = vertices_xyz; ref_nv = nv; ref_tris = faces; ref_nf = nf; }
    if ((rc = plan_args(vertices_xyz, nv, faces, nf, nullptr, 0, who))) return rc;
    if (ref_vertices != vertices_xyz || ref_tris != faces)
        if ((rc = plan_args(ref_vertices, ref_nv, ref_tris, ref_nf, nullptr, 0, who))) return rc;
    if (6 * nf > kMaxIndex) return set_error(MM_ERR_TOO_LARGE, "mm_mesh_relax: 6 nf passes 2^31");

    std::vector<uint8_t> flags;
    vertex_flags(faces, nf, nv, flags);
    mm_relax_report rep;
    std::memset(&rep, 0, sizeof(rep));
    rep.n_vertices = nv; rep.n_faces = nf; rep.n_ref_faces = ref_nf;
    rep.iterations_run = n_iterations;
    std::vector<int32_t> free_v;                                       // the free vertices, ascending
    for (int64_t v = 0; v < nv; ++v) {
        const bool pin = pinned && pinned[v];
        rep.n_pinned += pin;
        rep.n_border += (flags[(size_t)v] & 2) != 0;
        rep.n_isolated += !(flags[(size_t)v] & 1);
        if (flags[(size_t)v] == 1 && !pin) free_v.push_back((int32_t)v);
    }
    const int64_t nq = (int64_t)free_v.size();
    rep.n_free = nq;
    if (nq > 0 && ref_nf == 0) return set_error(MM_ERR_INVALID, "mm_mesh_relax: a free vertex and no reference face");

    auto copy_input = [&] {
        if (nv > 0 && out_vertices != vertices_xyz) std::memmove(out_vertices, vertices_xyz, (size_t)nv * 24);
        for (int64_t v = 0; v < nv; ++v) out_ref_face[v] = -1;
    };
    if (nv == 0 || nf == 0) {                                          // no edge: nothing is free, nothing is launched
        copy_input();
        *report = rep;
        return MM_OK;
    }

    // step 0's plan over the free vertices' input positions
    TriPlan pl;
    std::vector<double> qin((size_t)nq * 3);
    for (int64_t j = 0; j < nq; ++j) std::memcpy(&qin[(size_t)(3 * j)], vertices_xyz + 3 * (int64_t)free_v[(size_t)j], 24);
    if (nq > 0 && (rc = build_plan(ref_vertices, ref_tris, ref_nf, qin.data(), nq, who, pl))) return rc;
    const int64_t n_items = pl.n_a + pl.n_b, nch = (int64_t)pl.cbox.size();
    const bool project = nq > 0, iterate = project && n_iterations > 0;

    // device: [faces | v0 | staged reference | queries | their vertices | items | chunk boxes] (the upload),
    // [x | the queries' faces | numbers] (the download), then scratch
    const size_t vbytes = (size_t)nv * 24, V = (size_t)nv, Q = (size_t)nq;
    CsrDev d;
    const int32_t *d_face, *qv;
    const double *v0, *tri, *cbox;
    double *qxyz, *x, *cl, *sa, *sb;
    TriWork* work;
    unsigned long long *fkey, *num, *sq, *key;
    int32_t *reg, *vq;
    unsigned int* state;
    size_t o_face = 0, o_v0 = 0, o_tri = 0, o_q = 0, o_qv = 0, o_work = 0, o_cbox = 0, o_x = 0, o_fkey = 0, o_num = 0;
    size_t up_bytes = 0, down_bytes = 0;
    static_assert(relax_num_words * 8 <= 256 && sizeof(Box3) == 48, "the numbers block; six doubles a chunk box");
    rc = carve_on(e, e->dev_pts, [&](Carve& c) {
        o_face = c.place(d_face, 3 * (size_t)nf); o_v0 = c.place(v0, 3 * V);
        o_tri = c.place(tri, project ? 12 * (size_t)ref_nf : 0); o_q = c.place(qxyz, 3 * Q);
        o_qv = c.place(qv, Q); o_work = c.place(work, (size_t)n_items);
        o_cbox = c.place(cbox, 6 * (size_t)nch);
        up_bytes = c.size();
        o_x = c.place(x, 3 * V); o_fkey = c.place(fkey, Q); o_num = c.place(num, 32);
        down_bytes = c.size() - up_bytes;
        c.place(sq, Q); c.place(key, Q); c.place(cl, 3 * Q);
        c.place(reg, Q); c.place(state, Q); c.place(vq, V);
        if (iterate) d.lay(c, nf, nv);
        c.place(sa, (size_t)nf); c.place(sb, weld_sum_scratch(nf));
    });
    if (rc) return rc;
    if ((rc = e->ensure(e->host_pts, std::max(up_bytes, down_bytes) + 512, true))) return rc;
    unsigned char* hb = (unsigned char*)e->host_pts.p;
    unsigned char* b = (unsigned char*)e->dev_pts.p;
    d.counts = num + relax_num_csr;

    narrow_faces((int32_t*)(hb + o_face), faces, 3 * nf);
    std::memcpy(hb + o_v0, vertices_xyz, vbytes);
    if (project) {
        stage_tri_records(pl, ref_vertices, ref_tris, ref_nf, (double*)(hb + o_tri));
        double* hq = (double*)(hb + o_q);
        int32_t* hqv = (int32_t*)(hb + o_qv);
        for (int64_t j = 0; j < nq; ++j) {
            const int64_t i = pl.qperm[(size_t)j];
            std::memcpy(hq + 3 * j, &qin[(size_t)(3 * i)], 24);
            hqv[j] = free_v[(size_t)i];
        }
        std::memcpy(hb + o_work, pl.work.data(), (size_t)n_items * sizeof(TriWork));
        std::memcpy(hb + o_cbox, pl.cbox.data(), (size_t)nch * sizeof(Box3));
    }

    int launches = 0;
    MM_TRY_HIP(hipMemcpyAsync(b, hb, up_bytes, hipMemcpyHostToDevice, e->stream));
    MM_TRY_HIP(hipMemsetAsync(num, 0, 256, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(x, v0, vbytes, hipMemcpyDeviceToDevice, e->stream));
    MM_TRY_HIP(launch_weld_volume(v0, d_face, nf, sa, sb, (double*)(num + relax_num_vol_before), e->stream));
    if (project) {
        MM_TRY_HIP(hipMemsetAsync(vq, 0xFF, (size_t)nv * 4, e->stream));
        // step 0: fill, pass A, pass B, the who pass, the closest points; its own counter takes the items pass B skipped
        // on the host's bounds, apart from those the refreshed bounds skip
        MM_TRY_HIP(launch_tri_distance(work, (int)pl.n_a, (int)pl.n_b, tri, (int)ref_nf, qxyz, (int)nq, sq, key, cl, reg,
                                       num + relax_num_skipped0, e->stream));
        launches += tri_launches((int)pl.n_b);
        MM_TRY_HIP(launch_relax_accept(qv, (int)nq, cl, key, sq, x, fkey, vq, num, e->stream));
        ++launches;
    }
    if (iterate) {
        if ((rc = csr_build(e, d, d_face, nf, nv, &launches))) return rc;
        for (int64_t it = 0; it < n_iterations; ++it) {
            MM_TRY_HIP(launch_relax_candidates(d.off, d.nb, x, qv, (int)nq, fkey, tri, factor, qxyz, sq, key, state, work,
                                               (int)pl.n_a, (int)pl.n_b, cbox, e->stream));
            MM_TRY_HIP(launch_tri_seeded(work, (int)n_items, tri, (int)ref_nf, qxyz, (int)nq, sq, key, cl, reg,
                                         num + relax_num_skipped, e->stream));
            MM_TRY_HIP(launch_relax_guard(d_face, nf, x, cl, key, vq, state, e->stream));
            MM_TRY_HIP(launch_relax_apply(qv, (int)nq, cl, key, state, x, fkey, num, e->stream));
            launches += 3 + tri_seeded_launches();
        }
    }
    MM_TRY_HIP(launch_weld_volume(x, d_face, nf, sa, sb, (double*)(num + relax_num_vol_after), e->stream));
    launches += 2 * weld_volume_launches(nf);
    MM_TRY_HIP(launch_relax_flipped(d_face, nf, v0, x, num, e->stream));
    ++launches;
    MM_TRY_HIP(launch_mesh_disp(v0, x, nv, num + relax_num_disp, &launches, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(hb, x, down_bytes, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));

    std::memcpy(out_vertices, hb, vbytes);
    const unsigned long long* hkey = (const unsigned long long*)(hb + (o_fkey - o_x));
    for (int64_t v = 0; v < nv; ++v) out_ref_face[v] = -1;
    for (int64_t j = 0; j < nq; ++j)
        if (hkey[j] != ~0ull) out_ref_face[free_v[(size_t)pl.qperm[(size_t)j]]] = (int64_t)(hkey[j] >> 32);
    unsigned long long n[relax_num_words];
    std::memcpy(n, hb + (o_num - o_x), sizeof(n));
    double dn[relax_num_words];
    std::memcpy(dn, n, sizeof(n));
    rep.n_reverted = (int64_t)n[relax_num_reverted];
    rep.n_flipped_faces = (int64_t)n[relax_num_flipped];
    rep.items_skipped_step0 = (int64_t)n[relax_num_skipped0];
    rep.items_skipped = rep.items_skipped_step0 + (int64_t)n[relax_num_skipped];
    rep.items_run = n_items * (1 + n_iterations) - rep.items_skipped;
    rep.n_launches = launches;
    rep.bytes_uploaded = (int64_t)up_bytes;
    rep.bytes_downloaded = (int64_t)down_bytes;
    rep.initial_distance_sq = dn[relax_num_init];
    rep.max_displacement_sq = dn[relax_num_disp];
    rep.volume_before = dn[relax_num_vol_before] / 6.0;
    rep.volume_after = dn[relax_num_vol_after] / 6.0;
    *report = rep;
    return MM_OK;
}

}  // extern "C"
