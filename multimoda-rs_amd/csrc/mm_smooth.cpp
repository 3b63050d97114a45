// mm_smooth.cpp -- CCTA mesh finishing (include/mm_ccta.h, "mesh smoothing"): the sorted vertex adjacency, Laplacian /
// Taubin smoothing with a pin mask, ring distances from seed vertices.  Reference: multimodars/ccta/fixing_functions.py:
// 52-92 (the filter_taubin that ends the post-processing).  The host checks the arguments, narrows the faces to int32,
// lays the device buffers out and reads the report back; everything over the mesh runs on the device
// (mm_weld_kernels.hip for the edge table and the volume, mm_smooth_kernels.hip for the rest).
//
// mm_mesh_smooth keeps the input coordinates (v0) for the displacement and ping-pongs between two buffers (vA, vB): step
// 0 reads v0 and writes vA, every later step swaps vA and vB.  The report's numbers sit between vA and vB, so whichever
// of the two holds the result comes down together with them in one copy.
#include <algorithm>
#include <climits>
#include <cstring>

#include "../../include/mm_ccta.h"
#include "mm_stage.h"

using namespace mm;

extern "C" {

int mm_mesh_adjacency_csr(mm_engine* h, const int64_t* faces, int64_t nf, int64_t nv, int64_t nb_cap, int64_t* off,
                          int64_t* nb, int64_t* info)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (nb_cap < 0 || !off || !info || (nb_cap > 0 && !nb)) return set_error(MM_ERR_INVALID, "mm_mesh_adjacency_csr: bad arguments");
    if ((rc = mesh_args("mm_mesh_adjacency_csr", nullptr, nv, faces, nf, false))) return rc;
    std::memset(info, 0, 4 * sizeof(int64_t));
    if (nv == 0 || nf == 0) {
        for (int64_t i = 0; i <= nv; ++i) off[i] = 0;
        info[2] = nv;
        return MM_OK;
    }
    CsrDev d;
    int32_t* d_face;
    if ((rc = e->ensure(e->host_pts, (size_t)nf * 12 + 512, true))) return rc;
    rc = carve_on(e, e->dev_pts, [&](Carve& c) {
        c.place(d_face, 3 * (size_t)nf);
        d.lay(c, nf, nv);
        c.place(d.counts, 4);
    });
    if (rc) return rc;
    unsigned char* hb = (unsigned char*)e->host_pts.p;
    int32_t* hf = (int32_t*)hb;
    narrow_faces(hf, faces, 3 * nf);
    int launches = 0;
    MM_TRY_HIP(hipMemcpyAsync(d_face, hf, (size_t)nf * 12, hipMemcpyHostToDevice, e->stream));
    if ((rc = csr_build(e, d, d_face, nf, nv, &launches))) return rc;
    MM_TRY_HIP(hipMemcpyAsync(hb, d.counts, 4 * 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    const unsigned long long* c = (const unsigned long long*)hb;
    const int64_t entries = 2 * (int64_t)c[0];
    if (entries < 0 || entries > 6 * nf) return set_error(MM_ERR_HIP, "mm_mesh_adjacency_csr: entry count out of range");
    info[0] = entries; info[1] = (int64_t)c[2]; info[2] = (int64_t)c[1]; info[3] = launches;
    if (entries > nb_cap) return set_error(MM_ERR_TOO_LARGE, "mm_mesh_adjacency_csr: nb_cap too small (info[0] holds the size)");
    const size_t h_nb = up256(((size_t)nv + 1) * 4);
    if ((rc = e->ensure(e->host_pts, h_nb + (size_t)entries * 4 + 512, true))) return rc;
    hb = (unsigned char*)e->host_pts.p;
    MM_TRY_HIP(hipMemcpyAsync(hb, d.off, ((size_t)nv + 1) * 4, hipMemcpyDeviceToHost, e->stream));
    if (entries > 0) MM_TRY_HIP(hipMemcpyAsync(hb + h_nb, d.nb, (size_t)entries * 4, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    const int32_t* ho = (const int32_t*)hb;
    const int32_t* hn = (const int32_t*)(hb + h_nb);
    if (ho[nv] != entries) return set_error(MM_ERR_HIP, "mm_mesh_adjacency_csr: the scan and the edge count disagree");
    for (int64_t i = 0; i <= nv; ++i) off[i] = ho[i];
    for (int64_t k = 0; k < entries; ++k) nb[k] = hn[k];
    return MM_OK;
}

int mm_mesh_smooth(mm_engine* h, const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf,
                   const double* factors, int64_t n_steps, const uint8_t* pinned, double* out_vertices,
                   mm_smooth_report* report)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (!report || n_steps < 0 || (n_steps > 0 && !factors) || (nv > 0 && !out_vertices))
        return set_error(MM_ERR_INVALID, "mm_mesh_smooth: bad arguments");
    if ((rc = mesh_args("mm_mesh_smooth", vertices_xyz, nv, faces, nf, true))) return rc;
    std::memset(report, 0, sizeof(*report));
    report->n_vertices = nv;
    report->n_faces = nf;
    report->steps_run = n_steps;
    if (pinned)
        for (int64_t i = 0; i < nv; ++i) report->n_pinned += pinned[i] != 0;
    if (nv == 0 || nf == 0) {                                           // no edge: nothing moves
        report->n_isolated = nv;
        if (nv > 0) std::memmove(out_vertices, vertices_xyz, (size_t)nv * 24);
        return MM_OK;
    }

    // device: [faces | mask | v0] (the upload), vA, the report's numbers, vB, the adjacency, the volume's scratch
    const size_t vbytes = (size_t)nv * 24, V = (size_t)nv;
    CsrDev d;
    const int32_t* d_face;
    const uint8_t* d_mask;
    const double* v0;
    double *va, *vb, *d_num, *sa, *sb;
    size_t o_face = 0, o_mask = 0, o_v0 = 0, o_va = 0, o_num = 0, o_vb = 0;
    rc = carve_on(e, e->dev_pts, [&](Carve& c) {
        o_face = c.place(d_face, 3 * (size_t)nf); o_mask = c.place(d_mask, pinned ? V : 0); o_v0 = c.place(v0, 3 * V);
        o_va = c.place(va, 3 * V); o_num = c.place(d_num, 32); o_vb = c.place(vb, 3 * V);
        d.lay(c, nf, nv);
        c.place(sa, (size_t)nf); c.place(sb, weld_sum_scratch(nf));
    });
    if (rc) return rc;
    const size_t up_bytes = o_v0 + vbytes, down_bytes = o_vb + vbytes - o_va;
    if ((rc = e->ensure(e->host_pts, std::max(up_bytes, down_bytes) + 512, true))) return rc;
    unsigned char* hb = (unsigned char*)e->host_pts.p;
    unsigned char* b = (unsigned char*)e->dev_pts.p;
    enum { kVolBefore = 0, kVolAfter = 1, kDisp = 2, kCounts = 3 };    // 8-byte words of the numbers block (32 of them)
    d.counts = (unsigned long long*)(d_num + kCounts);
    if (!pinned) d_mask = nullptr;
    int32_t* hf = (int32_t*)(hb + o_face);
    narrow_faces(hf, faces, 3 * nf);
    if (pinned) std::memcpy(hb + o_mask, pinned, V);
    std::memcpy(hb + o_v0, vertices_xyz, vbytes);
    int launches = 0;
    MM_TRY_HIP(hipMemcpyAsync(b, hb, up_bytes, hipMemcpyHostToDevice, e->stream));
    if ((rc = csr_build(e, d, d_face, nf, nv, &launches))) return rc;
    MM_TRY_HIP(launch_weld_volume(v0, d_face, nf, sa, sb, d_num + kVolBefore, e->stream));
    const double* cur = v0;
    for (int64_t i = 0; i < n_steps; ++i) {
        double* next = cur == va ? vb : va;
        MM_TRY_HIP(launch_mesh_step(d.off, d.nb, cur, next, nv, factors[i], d_mask, &launches, e->stream));
        cur = next;
    }
    MM_TRY_HIP(launch_weld_volume(cur, d_face, nf, sa, sb, d_num + kVolAfter, e->stream));
    launches += 2 * weld_volume_launches(nf);
    MM_TRY_HIP(launch_mesh_disp(v0, cur, nv, (unsigned long long*)(d_num + kDisp), &launches, e->stream));
    // one copy down: [vA | numbers] or [numbers | vB], whichever holds the result; the numbers alone without a step
    const size_t from = cur == va ? o_va : o_num;
    const size_t bytes = cur == va ? o_num + 256 - o_va : (cur == vb ? o_vb + vbytes - o_num : 256);
    MM_TRY_HIP(hipMemcpyAsync(hb, b + from, bytes, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    const double* num = (const double*)(hb + (o_num - from));
    if (cur == v0) std::memmove(out_vertices, vertices_xyz, vbytes);
    else std::memcpy(out_vertices, hb + ((cur == va ? o_va : o_vb) - from), vbytes);
    unsigned long long c[4];
    std::memcpy(c, num + kCounts, sizeof(c));
    report->n_edges = (int64_t)c[0];
    report->n_isolated = (int64_t)c[1];
    report->max_degree = (int64_t)c[2];
    report->launches = launches;
    report->volume_before = num[kVolBefore] / 6.0;
    report->volume_after = num[kVolAfter] / 6.0;
    report->max_displacement_sq = num[kDisp];
    return MM_OK;
}

int mm_mesh_vertex_rings(mm_engine* h, const int64_t* faces, int64_t nf, int64_t nv, const int64_t* seeds,
                         int64_t n_seeds, int64_t max_ring, int32_t* ring_out, int64_t* info)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (!info || n_seeds < 0 || n_seeds > kMaxIndex || max_ring < 0 || (n_seeds > 0 && !seeds) || (nv > 0 && !ring_out))
        return set_error(MM_ERR_INVALID, "mm_mesh_vertex_rings: bad arguments");
    if ((rc = mesh_args("mm_mesh_vertex_rings", nullptr, nv, faces, nf, false))) return rc;
    for (int64_t k = 0; k < n_seeds; ++k)
        if (seeds[k] < 0 || seeds[k] >= nv) return set_error(MM_ERR_INVALID, "mm_mesh_vertex_rings: seed out of range");
    std::memset(info, 0, 3 * sizeof(int64_t));
    if (nv == 0) return MM_OK;
    if (nf == 0 || n_seeds == 0) {                                      // no edge or no seed: the seeds alone
        for (int64_t i = 0; i < nv; ++i) ring_out[i] = -1;
        for (int64_t k = 0; k < n_seeds; ++k) {
            info[0] += ring_out[seeds[k]] == -1;
            ring_out[seeds[k]] = 0;
        }
        return MM_OK;
    }
    CsrDev d;
    const int32_t *d_face, *d_seed;
    int32_t* d_ring;
    unsigned long long* d_reached;
    size_t o_seed = 0;
    rc = carve_on(e, e->dev_pts, [&](Carve& c) {
        c.place(d_face, 3 * (size_t)nf); o_seed = c.place(d_seed, (size_t)n_seeds);
        d.lay(c, nf, nv);
        c.place(d_ring, (size_t)nv); c.place(d.counts, 4); c.place(d_reached, 1);
    });
    if (rc) return rc;
    const size_t up_bytes = o_seed + (size_t)n_seeds * 4;
    const size_t h_flag = up256(std::max(up_bytes, (size_t)nv * 4));   // the round's count, behind upload and download
    if ((rc = e->ensure(e->host_pts, h_flag + 512, true))) return rc;
    unsigned char* hb = (unsigned char*)e->host_pts.p;
    narrow_faces((int32_t*)hb, faces, 3 * nf);
    int32_t* hs = (int32_t*)(hb + o_seed);
    for (int64_t k = 0; k < n_seeds; ++k) hs[k] = (int32_t)seeds[k];
    const unsigned long long* h_reached = (const unsigned long long*)(hb + h_flag);
    int launches = 0;
    MM_TRY_HIP(hipMemcpyAsync(e->dev_pts.p, hb, up_bytes, hipMemcpyHostToDevice, e->stream));
    if ((rc = csr_build(e, d, d_face, nf, nv, &launches))) return rc;
    MM_TRY_HIP(launch_mesh_ring_seed(d_seed, n_seeds, d_ring, nv, d_reached, &launches, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(hb + h_flag, d_reached, 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    int64_t reached = (int64_t)h_reached[0], rounds = 0;
    for (int64_t r = 1; r <= max_ring; ++r) {                           // a round that reaches nothing is the last
        MM_TRY_HIP(launch_mesh_ring(d.off, d.nb, nv, d_ring, (int32_t)r, d_reached, &launches, e->stream));
        MM_TRY_HIP(hipMemcpyAsync(hb + h_flag, d_reached, 8, hipMemcpyDeviceToHost, e->stream));
        MM_TRY_HIP(hipStreamSynchronize(e->stream));
        ++rounds;
        const int64_t now = (int64_t)h_reached[0];
        if (now == reached) break;
        reached = now;
    }
    MM_TRY_HIP(hipMemcpyAsync(hb, d_ring, (size_t)nv * 4, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    std::memcpy(ring_out, hb, (size_t)nv * 4);
    info[0] = reached; info[1] = rounds; info[2] = launches;
    return MM_OK;
}

}  // extern "C"
