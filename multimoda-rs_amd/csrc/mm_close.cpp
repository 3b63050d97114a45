// mm_close.cpp -- CCTA mesh closing (include/mm_ccta.h): hole filling and label smoothing.  Reference:
// multimodars/ccta/fixing_functions.py:13-49 (manual_hole_fill), src/ccta/binding/ccta_py.rs:743-814
// (smooth_mesh_labels).  What runs over every face or vertex -- the edge table, the winding, the open half-edges, the
// fans, the volume, the edge report, the votes -- runs on the device (mm_weld_kernels.hip, mm_close_kernels.hip); the
// walk over the rim touches a few hundred to a few thousand edges and is host C++ here, as the ring logic of the
// trimming is.
//
// mm_fill_holes works in two phases.  The first is sized by the input: faces up, winding, the open half-edges down.
// The walk then says how large the result is, and the second phase is sized by exactly that: the wound faces move
// device to device in front of the fans, the table is rebuilt over all of them for the edge report, the volume is
// summed.  Nothing is sized for the worst case (3 nf fan faces).  The vertices are not changed by any stage, so the
// result's vertices are written on the host from the input and the centroids; they go to the device only for the volume.
#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "../../include/mm_ccta.h"
#include "mm_stage.h"

namespace mm {
namespace {

// ---- the walk over the rim (host) -------------------------------------------------------------------------------------

struct Loops {
    std::vector<int64_t> len, idx;       // the loops of at least 3 vertices, back to back
    int64_t irregular_components = 0, irregular_edges = 0, short_loops = 0;
};

// half_edges: ne (a, b) pairs, checked by the caller
void walk_loops(const int64_t* he, int64_t ne, Loops& out)
{
    std::vector<int64_t> verts((size_t)(2 * ne));
    for (int64_t k = 0; k < 2 * ne; ++k) verts[(size_t)k] = he[k];
    std::sort(verts.begin(), verts.end());
    verts.erase(std::unique(verts.begin(), verts.end()), verts.end());
    const size_t n = verts.size();
    auto local = [&](int64_t v) { return (size_t)(std::lower_bound(verts.begin(), verts.end(), v) - verts.begin()); };
    std::vector<int32_t> n_out(n, 0), n_in(n, 0);
    std::vector<size_t> succ(n, 0), parent(n);
    for (size_t i = 0; i < n; ++i) parent[i] = i;
    auto find = [&](size_t x) {
        while (parent[x] != x) { parent[x] = parent[parent[x]]; x = parent[x]; }
        return x;
    };
    std::vector<size_t> tail((size_t)ne);
    for (int64_t k = 0; k < ne; ++k) {
        const size_t a = local(he[2 * k]), b = local(he[2 * k + 1]);
        tail[(size_t)k] = a;
        ++n_out[a];
        ++n_in[b];
        succ[a] = b;
        const size_t ra = find(a), rb = find(b);
        if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb);
    }
    std::vector<uint8_t> irregular(n, 0);                  // by component root
    for (size_t i = 0; i < n; ++i)
        if (n_out[i] != 1 || n_in[i] != 1) irregular[find(i)] = 1;
    for (size_t i = 0; i < n; ++i)
        if (find(i) == i && irregular[i]) ++out.irregular_components;
    for (int64_t k = 0; k < ne; ++k)
        if (irregular[find(tail[(size_t)k])]) ++out.irregular_edges;
    std::vector<uint8_t> seen(n, 0);
    for (size_t i = 0; i < n; ++i) {                       // ascending local index = ascending vertex index
        if (seen[i] || irregular[find(i)]) continue;
        const size_t at = out.idx.size();
        size_t x = i;
        do {
            seen[x] = 1;
            out.idx.push_back(verts[x]);
            x = succ[x];
        } while (x != i);
        const int64_t len = (int64_t)(out.idx.size() - at);
        if (len < 3) { out.idx.resize(at); ++out.short_loops; }
        else out.len.push_back(len);
    }
}

// the sequential sum of the loop's points in walk order, per coordinate, divided by their number
void loop_centroid(const double* v, const int64_t* idx, int64_t n, double out[3])
{
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t i = 0; i < n; ++i)
        for (int c = 0; c < 3; ++c) s[c] += v[3 * idx[i] + c];
    for (int c = 0; c < 3; ++c) out[c] = s[c] / (double)n;
}

// the shared front of the two smoothing entry points
int smooth_args(mm_engine* h, Engine*& e, const uint8_t* labels, int64_t nv, int64_t iterations, uint8_t* out_labels,
                int64_t* info, const char* who)
{
    const int rc = engine_of(h, e);
    if (rc) return rc;
    if (nv < 0 || nv > kMaxIndex || iterations < 0 || !info || (nv > 0 && (!labels || !out_labels)))
        return set_error(MM_ERR_INVALID, std::string(who) + ": bad arguments");
    return MM_OK;
}

// The iterations of either form.  Device layout behind `topo_bytes` of topology (uploaded from the pinned buffer with the
// labels): cur, next (nv bytes each), vote (nv words, faces form only), the flip counter.
int smooth_run(Engine* e, const uint8_t* labels, int64_t nv, size_t topo_bytes, bool csr, int64_t n_a, int64_t iterations,
               uint8_t* out_labels, int64_t* info)
{
    // pinned: [topology | labels | counter]; device: [topology | labels = cur | next | vote | counter]
    const size_t h_lab = up256(topo_bytes), h_cnt = up256(h_lab + (size_t)nv);
    const size_t o_next = up256(h_lab + (size_t)nv), o_vote = up256(o_next + (size_t)nv);
    const size_t o_cnt = up256(o_vote + (csr ? 0 : (size_t)nv * 4)), dev_bytes = o_cnt + 256;
    unsigned char* hb = (unsigned char*)e->host_pts.p;               // ensured by the caller: h_cnt + 256 at least
    int rc;
    if ((rc = e->ensure(e->dev_pts, dev_bytes, false))) return rc;
    unsigned char* b = (unsigned char*)e->dev_pts.p;
    std::memcpy(hb + h_lab, labels, (size_t)nv);
    uint8_t *cur = b + h_lab, *next = b + o_next;
    unsigned int* vote = (unsigned int*)(b + o_vote);
    unsigned long long* d_cnt = (unsigned long long*)(b + o_cnt);
    unsigned long long* h_flips = (unsigned long long*)(hb + h_cnt);
    MM_TRY_HIP(hipMemcpyAsync(b, hb, h_lab + (size_t)nv, hipMemcpyHostToDevice, e->stream));
    if (!csr) MM_TRY_HIP(hipMemsetAsync(vote, 0, (size_t)nv * 4, e->stream));
    MM_TRY_HIP(hipMemsetAsync(d_cnt, 0, 8, e->stream));
    int launches = 0;
    int64_t it = 0, total = 0, last = 0;
    const int32_t* topo = (const int32_t*)b;
    while (it < iterations) {
        if (csr) MM_TRY_HIP(launch_smooth_csr(topo, topo + (nv + 1), nv, cur, next, d_cnt, &launches, e->stream));
        else MM_TRY_HIP(launch_smooth_faces(topo, n_a, nv, cur, vote, next, d_cnt, &launches, e->stream));
        MM_TRY_HIP(hipMemcpyAsync(h_flips, d_cnt, 8, hipMemcpyDeviceToHost, e->stream));
        MM_TRY_HIP(hipStreamSynchronize(e->stream));
        ++it;
        last = (int64_t)h_flips[0] - total;
        total = (int64_t)h_flips[0];
        std::swap(cur, next);
        if (last == 0) break;
    }
    MM_TRY_HIP(hipMemcpyAsync(hb + h_lab, cur, (size_t)nv, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    std::memcpy(out_labels, hb + h_lab, (size_t)nv);
    info[0] = it; info[1] = total; info[2] = last; info[3] = launches;
    return MM_OK;
}

}  // namespace
}  // namespace mm

using namespace mm;

extern "C" {

int mm_hole_loops(const int64_t* half_edges, int64_t ne, const double* vertices_xyz, int64_t nv, int64_t* loop_len,
                  int64_t* loop_idx, double* centroids, int64_t* counts)
{
    if (ne < 0 || nv < 0 || ne > kMaxIndex || !counts || (ne > 0 && (!half_edges || !loop_len || !loop_idx)) ||
        (centroids && !vertices_xyz))
        return set_error(MM_ERR_INVALID, "mm_hole_loops: bad arguments");
    for (int64_t k = 0; k < 2 * ne; ++k)
        if (half_edges[k] < 0 || half_edges[k] >= nv) return set_error(MM_ERR_INVALID, "mm_hole_loops: vertex index out of range");
    Loops lp;
    walk_loops(half_edges, ne, lp);
    int64_t at = 0;
    for (size_t k = 0; k < lp.len.size(); ++k) {
        loop_len[k] = lp.len[k];
        if (centroids) loop_centroid(vertices_xyz, &lp.idx[(size_t)at], lp.len[k], centroids + 3 * k);
        at += lp.len[k];
    }
    for (size_t k = 0; k < lp.idx.size(); ++k) loop_idx[k] = lp.idx[k];
    counts[0] = (int64_t)lp.len.size();
    counts[1] = (int64_t)lp.idx.size();
    counts[2] = lp.irregular_components;
    counts[3] = lp.irregular_edges;
    counts[4] = lp.short_loops;
    return MM_OK;
}

int mm_fill_holes(mm_engine* h, const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf, int fix_normals,
                  int64_t vert_cap, int64_t face_cap, double* out_vertices, int64_t* out_faces, mm_fill_report* report)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (nv < 0 || nf < 0 || nv > kMaxIndex || nf > kMaxIndex || !report || vert_cap < 0 || face_cap < 0 ||
        (nv > 0 && !vertices_xyz) || (nf > 0 && !faces) || (vert_cap > 0 && !out_vertices) || (face_cap > 0 && !out_faces))
        return set_error(MM_ERR_INVALID, "mm_fill_holes: bad arguments");
    if ((rc = faces_in_range(faces, nf, nv, "mm_fill_holes"))) return rc;
    std::memset(report, 0, sizeof(*report));
    const bool fix = fix_normals != 0;
    if (nf == 0) {                                                    // no face, no rim
        report->n_vertices = nv;
        if (vert_cap < nv) return set_error(MM_ERR_TOO_LARGE, "mm_fill_holes: vert_cap too small");
        if (nv > 0) std::memcpy(out_vertices, vertices_xyz, (size_t)nv * 24);
        return MM_OK;
    }

    // ---- phase 1 (dev_pts): faces up, winding, open half-edges down
    enum { kFlipped = 0, kOpen = 1, kNonManifold = 2, kConflict = 3, kOpen2 = 4, kNonManifold2 = 5, kConflict2 = 6, kCounts = 8 };
    EdgeTable t;
    int32_t* d_face;
    unsigned int *d_link, *d_changed;
    unsigned long long *d_counts, *d_list, *d_nlist;
    if ((rc = e->ensure(e->host_pts, (size_t)nf * 24 + 512, true))) return rc;
    rc = carve_on(e, e->dev_pts, [&](Carve& c) {
        c.place(d_face, 3 * (size_t)nf);
        t.lay(c, nf);
        c.place(d_link, (size_t)nf); c.place(d_list, 3 * (size_t)nf); c.place(d_nlist, 1);
        c.place(d_counts, kCounts); c.place(d_changed, 1);
    });
    if (rc) return rc;
    unsigned char* hb = (unsigned char*)e->host_pts.p;
    int32_t* hf = (int32_t*)hb;
    narrow_faces(hf, faces, 3 * nf);
    WindDev w{t.keys, t.cnt, t.own, d_link, d_changed, d_counts + kFlipped, d_counts + kOpen, t.log2_e};
    MM_TRY_HIP(hipMemcpyAsync(d_face, hf, (size_t)nf * 12, hipMemcpyHostToDevice, e->stream));
    MM_TRY_HIP(hipMemsetAsync(d_counts, 0, kCounts * 8, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));                      // the pinned buffer takes the round flags next
    int64_t rounds = 0;
    if ((rc = weld_wind(e, w, d_face, nf, fix, &rounds))) return rc;
    MM_TRY_HIP(launch_close_half_edges(w.keys, w.cnt, w.own, w.log2_e, fix ? w.link : nullptr, d_list,
                                       3ull * (unsigned long long)nf, d_nlist, e->stream));
    unsigned long long* h_n = (unsigned long long*)hb;
    MM_TRY_HIP(hipMemcpyAsync(h_n, d_nlist, 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(h_n + 1, d_counts, kCounts * 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    const int64_t n_open = (int64_t)h_n[0];
    const int64_t n_flipped = (int64_t)h_n[1 + kFlipped];
    if (n_open < 0 || n_open > 3 * nf || n_open != (int64_t)h_n[1 + kOpen])
        return set_error(MM_ERR_HIP, "mm_fill_holes: open edge count out of range");
    std::vector<int64_t> he((size_t)(2 * n_open));
    if (n_open > 0) {
        MM_TRY_HIP(hipMemcpyAsync(hb, d_list, (size_t)n_open * 8, hipMemcpyDeviceToHost, e->stream));
        MM_TRY_HIP(hipStreamSynchronize(e->stream));
        const unsigned long long* hl = (const unsigned long long*)hb;
        for (int64_t k = 0; k < n_open; ++k) {
            he[(size_t)(2 * k)] = (int64_t)(hl[k] >> 32);
            he[(size_t)(2 * k + 1)] = (int64_t)(hl[k] & 0xFFFFFFFFull);
            if (he[(size_t)(2 * k)] >= nv || he[(size_t)(2 * k + 1)] >= nv)
                return set_error(MM_ERR_HIP, "mm_fill_holes: half-edge out of range");
        }
    }

    // ---- the walk (host)
    Loops lp;
    walk_loops(he.data(), n_open, lp);
    const int64_t n_loops = (int64_t)lp.len.size(), n_fan = (int64_t)lp.idx.size();
    const int64_t nv2 = nv + n_loops, nf2 = nf + n_fan;
    report->n_loops_filled = n_loops;
    report->n_fan_faces = n_fan;
    report->n_open_edges_before = n_open;
    report->n_short_loops = lp.short_loops;
    report->n_irregular_components = lp.irregular_components;
    report->n_irregular_edges = lp.irregular_edges;
    report->n_flipped_faces = n_flipped;
    report->winding_rounds = rounds;
    report->n_vertices = nv2;
    report->n_faces = nf2;
    if (nv2 > kMaxIndex || nf2 > kMaxIndex) return set_error(MM_ERR_TOO_LARGE, "mm_fill_holes: the result passes 2^31");
    if (vert_cap < nv2 || face_cap < nf2)
        return set_error(MM_ERR_TOO_LARGE, "mm_fill_holes: vert_cap / face_cap too small (the report holds the sizes)");

    // ---- phase 2 (dev_lvl): sized by the result
    EdgeTable t2;
    const int32_t* d_fan;
    int32_t* d_face2;
    double *d_vert, *d_sa, *d_sb, *d_vol;
    size_t p_fan = 0, p_vert = 0, up_bytes = 0;
    rc = carve_on(e, e->dev_lvl, [&](Carve& c) {
        p_fan = c.place(d_fan, 3 * (size_t)n_fan); p_vert = c.place(d_vert, fix ? 3 * (size_t)nv2 : 0);
        up_bytes = c.size();
        c.place(d_face2, 3 * (size_t)nf2);
        t2.lay(c, nf2);
        c.place(d_sa, fix ? (size_t)nf2 : 0); c.place(d_sb, fix ? weld_sum_scratch(nf2) : 0);
        c.place(d_vol, 1);
    });
    if (rc) return rc;
    if ((rc = e->ensure(e->host_pts, std::max(up_bytes, (size_t)nf2 * 12) + 512, true))) return rc;
    hb = (unsigned char*)e->host_pts.p;
    int32_t* h_fan = (int32_t*)(hb + p_fan);
    std::vector<double> centroids((size_t)(3 * n_loops));
    {
        int64_t at = 0;
        for (int64_t k = 0; k < n_loops; ++k) {
            const int64_t n = lp.len[(size_t)k];
            loop_centroid(vertices_xyz, &lp.idx[(size_t)at], n, &centroids[(size_t)(3 * k)]);
            for (int64_t i = 0; i < n; ++i) {
                h_fan[3 * (at + i)] = (int32_t)lp.idx[(size_t)(at + i)];
                h_fan[3 * (at + i) + 1] = (int32_t)lp.idx[(size_t)(at + (i + 1) % n)];
                h_fan[3 * (at + i) + 2] = (int32_t)k;
            }
            at += n;
        }
    }
    if (fix) {
        std::memcpy(hb + p_vert, vertices_xyz, (size_t)nv * 24);
        if (n_loops > 0) std::memcpy(hb + p_vert + (size_t)nv * 24, centroids.data(), (size_t)n_loops * 24);
    }
    if (up_bytes > 0) MM_TRY_HIP(hipMemcpyAsync(e->dev_lvl.p, hb, up_bytes, hipMemcpyHostToDevice, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(d_face2, d_face, (size_t)nf * 12, hipMemcpyDeviceToDevice, e->stream));
    MM_TRY_HIP(launch_close_fan(d_fan, n_fan, nv, d_face2, nf, e->stream));
    MM_TRY_HIP(launch_weld_edges(d_face2, nf2, t2.keys, t2.cnt, t2.own, t2.log2_e, e->stream));
    MM_TRY_HIP(launch_weld_edge_report(t2.keys, t2.cnt, t2.own, t2.log2_e, nullptr, d_counts + kOpen2, e->stream));
    double volume = 0.0;
    int inverted = 0;
    if (fix) {
        MM_TRY_HIP(launch_weld_volume(d_vert, d_face2, nf2, d_sa, d_sb, d_vol, e->stream));
        double* hv = (double*)hb;                                     // stream order: behind the upload from there
        MM_TRY_HIP(hipMemcpyAsync(hv, d_vol, 8, hipMemcpyDeviceToHost, e->stream));
        MM_TRY_HIP(hipStreamSynchronize(e->stream));
        volume = hv[0] / 6.0;
        if (volume < 0.0) {
            inverted = 1;
            MM_TRY_HIP(launch_weld_reverse(d_face2, nf2, e->stream));
        }
    }
    const size_t h_counts = up256((size_t)nf2 * 12);
    MM_TRY_HIP(hipMemcpyAsync(hb, d_face2, (size_t)nf2 * 12, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(hb + h_counts, d_counts, kCounts * 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    const int32_t* f32 = (const int32_t*)hb;
    widen_faces(out_faces, f32, 3 * nf2);
    if (nv > 0) std::memcpy(out_vertices, vertices_xyz, (size_t)nv * 24);
    if (n_loops > 0) std::memcpy(out_vertices + 3 * nv, centroids.data(), (size_t)n_loops * 24);
    const unsigned long long* c = (const unsigned long long*)(hb + h_counts);
    report->n_open_edges = (int64_t)c[kOpen2];
    report->n_nonmanifold_edges = (int64_t)c[kNonManifold2];
    report->inverted = inverted;
    report->volume = volume;
    return MM_OK;
}

int mm_smooth_labels_faces(mm_engine* h, const uint8_t* labels, int64_t nv, const int64_t* faces, int64_t nf,
                           int64_t iterations, uint8_t* out_labels, int64_t* info)
{
    Engine* e;
    int rc = smooth_args(h, e, labels, nv, iterations, out_labels, info, "mm_smooth_labels_faces");
    if (rc) return rc;
    if (nf < 0 || nf > kMaxIndex || (nf > 0 && !faces)) return set_error(MM_ERR_INVALID, "mm_smooth_labels_faces: bad arguments");
    if ((rc = faces_in_range(faces, nf, nv, "mm_smooth_labels_faces"))) return rc;
    std::memset(info, 0, 4 * sizeof(int64_t));
    if (nv == 0) return MM_OK;
    if (iterations == 0) { std::memmove(out_labels, labels, (size_t)nv); return MM_OK; }
    const size_t topo = (size_t)nf * 12;
    if ((rc = e->ensure(e->host_pts, up256(up256(topo) + (size_t)nv) + 512, true))) return rc;
    int32_t* hf = (int32_t*)e->host_pts.p;
    narrow_faces(hf, faces, 3 * nf);
    return smooth_run(e, labels, nv, topo, false, nf, iterations, out_labels, info);
}

int mm_smooth_labels_csr(mm_engine* h, const uint8_t* labels, int64_t nv, const int64_t* off, const int64_t* nb,
                         int64_t iterations, uint8_t* out_labels, int64_t* info)
{
    Engine* e;
    int rc = smooth_args(h, e, labels, nv, iterations, out_labels, info, "mm_smooth_labels_csr");
    if (rc) return rc;
    if (nv > 0 && !off) return set_error(MM_ERR_INVALID, "mm_smooth_labels_csr: bad arguments");
    std::memset(info, 0, 4 * sizeof(int64_t));
    if (nv == 0) return MM_OK;
    if (off[0] != 0) return set_error(MM_ERR_INVALID, "mm_smooth_labels_csr: offsets must start at 0");
    for (int64_t i = 0; i < nv; ++i)
        if (off[i + 1] < off[i] || off[i + 1] > kMaxIndex)
            return set_error(MM_ERR_INVALID, "mm_smooth_labels_csr: offsets must ascend and stay below 2^31");
    const int64_t nn = off[nv];
    if (nn > 0 && !nb) return set_error(MM_ERR_INVALID, "mm_smooth_labels_csr: bad arguments");
    for (int64_t k = 0; k < nn; ++k)
        if (nb[k] < 0 || nb[k] >= nv) return set_error(MM_ERR_INVALID, "mm_smooth_labels_csr: neighbour index out of range");
    if (iterations == 0) { std::memmove(out_labels, labels, (size_t)nv); return MM_OK; }
    const size_t topo = ((size_t)nv + 1 + (size_t)nn) * 4;
    if ((rc = e->ensure(e->host_pts, up256(up256(topo) + (size_t)nv) + 512, true))) return rc;
    int32_t* ht = (int32_t*)e->host_pts.p;
    for (int64_t i = 0; i <= nv; ++i) ht[i] = (int32_t)off[i];
    for (int64_t k = 0; k < nn; ++k) ht[nv + 1 + k] = (int32_t)nb[k];
    return smooth_run(e, labels, nv, topo, true, nn, iterations, out_labels, info);
}

}  // extern "C"
