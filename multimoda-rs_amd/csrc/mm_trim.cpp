// mm_trim.cpp -- CCTA mesh trimming (include/mm_ccta.h): cutting labelled regions out of a mesh, keeping only some of
// them, and tracing the open rim the cut leaves.  Reference: multimodars/ccta/boundary.py:26-325 (open-boundary rings),
// multimodars/ccta/stitching.py:110-352 (remove / keep), multimodars/ccta/__init__.py:341-373 (region with its border
// faces).  Everything that runs over every face -- region membership, rim seeds, open-edge counting, compaction -- runs
// on the device (mm_trim_kernels.hip); the ring logic on the rim (a few hundred vertices) is host C++ here.
//
// The reference walks its rim graph in CPython set order.  Here the rule is fixed (and restated in
// tests/mm_checkers/trim_mesh.py): rings are discovered in increasing order of their smallest remaining vertex, each
// starts at it, and from every vertex the walk goes to the smallest neighbour that is not the previous vertex and still
// remains; length ties keep discovery order.  Distances and cosines are (x*x + y*y) + z*z sums, unfused.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <iterator>
#include <string>
#include <vector>

#include "../../include/mm_ccta.h"
#include "mm_adjacency.h"
#include "mm_stage.h"

namespace mm {
namespace {

// ---- ring logic on the rim (host) -----------------------------------------------------------------------------------

using Ring = std::vector<int64_t>;

inline double dist3(const double* a, const double* b)
{
    const double dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return std::sqrt(dx * dx + dy * dy + dz * dz);
}

// _despike_ring (boundary.py:126-159): the ring without the vertices whose two edge directions have a cosine above
// cos_thresh, one at a time from the front, while more than 3 remain
Ring despike(Ring pts, const double* v, double cos_thresh)
{
    bool changed = true;
    while (changed && pts.size() > 3) {
        changed = false;
        const size_t m = pts.size();
        for (size_t i = 0; i < m; ++i) {
            const double* p = v + 3 * pts[i];
            const double* a = v + 3 * pts[(i + m - 1) % m];
            const double* b = v + 3 * pts[(i + 1) % m];
            const double d1x = a[0] - p[0], d1y = a[1] - p[1], d1z = a[2] - p[2];
            const double d2x = b[0] - p[0], d2y = b[1] - p[1], d2z = b[2] - p[2];
            const double n1 = std::sqrt(d1x * d1x + d1y * d1y + d1z * d1z);
            const double n2 = std::sqrt(d2x * d2x + d2y * d2y + d2z * d2z);
            if (n1 == 0.0 || n2 == 0.0) continue;
            if ((d1x * d2x + d1y * d2y + d1z * d2z) / (n1 * n2) > cos_thresh) {
                pts.erase(pts.begin() + (ptrdiff_t)i);
                changed = true;
                break;
            }
        }
    }
    return pts;
}

// _join_rings (boundary.py:162-190): merge the closest endpoints of different arcs (strict <, the reference's loop order)
// until target_n remain
std::vector<Ring> join_rings(std::vector<Ring> comps, const double* v, size_t target_n)
{
    while (comps.size() > target_n) {
        double best_dist = INFINITY;
        size_t ba = 0, bb = 1;
        bool bfa = false, bfb = false;
        for (size_t a = 0; a < comps.size(); ++a)
            for (size_t b = a + 1; b < comps.size(); ++b) {
                const std::pair<int64_t, bool> ea[2] = {{comps[a].front(), true}, {comps[a].back(), false}};
                const std::pair<int64_t, bool> eb[2] = {{comps[b].front(), false}, {comps[b].back(), true}};
                for (const auto& pa : ea)
                    for (const auto& pb : eb) {
                        const double d = dist3(v + 3 * pa.first, v + 3 * pb.first);
                        if (d < best_dist) { best_dist = d; ba = a; bb = b; bfa = pa.second; bfb = pb.second; }
                    }
            }
        Ring ca = comps[ba], cb = comps[bb];
        if (bfa) std::reverse(ca.begin(), ca.end());
        if (bfb) std::reverse(cb.begin(), cb.end());
        std::vector<Ring> next;
        for (size_t k = 0; k < comps.size(); ++k)
            if (k != ba && k != bb) next.push_back(std::move(comps[k]));
        ca.insert(ca.end(), cb.begin(), cb.end());
        next.push_back(std::move(ca));
        comps = std::move(next);
    }
    return comps;
}

void sort_by_length(std::vector<Ring>& r)
{
    std::stable_sort(r.begin(), r.end(), [](const Ring& a, const Ring& b) { return a.size() > b.size(); });
}

// _reduce_rings (boundary.py:193-215); target_n < 0: all rings
std::vector<Ring> reduce_rings(std::vector<Ring> rings, const double* v, int64_t target_n)
{
    rings.erase(std::remove_if(rings.begin(), rings.end(), [](const Ring& r) { return r.empty(); }), rings.end());
    sort_by_length(rings);
    if (target_n < 0 || (int64_t)rings.size() <= target_n) return rings;
    rings = join_rings(std::move(rings), v, (size_t)target_n);
    sort_by_length(rings);
    rings.resize((size_t)target_n);
    return rings;
}

// One pass of the rim logic over an open-edge list.  clean == false: order_boundary_rings (boundary.py:223-254) and the
// last re-derivation of clean_open_boundary.  clean == true: one round of clean_open_boundary (:298-321): `rim` = the
// vertices of the rims touching the seeds (empty: no rim, no rings), then either `drop` (the vertices of degree != 2, or
// else the despike spikes) or the reduced rings.  All outputs are ascending vertex indices except the rings.
struct RimResult {
    std::vector<int64_t> rim, drop;
    std::vector<Ring> rings;
};

void rim_pass(const int64_t* edges, int64_t ne, const std::vector<int64_t>& seeds, bool have_seeds, const double* v,
              int64_t target_n, double despike_cos, bool clean, RimResult& out)
{
    out = RimResult();
    // _boundary_graph (:54-64) on dense ids in vertex order; a (v, v) edge makes v its own neighbour once
    std::vector<int64_t> ids(edges, edges + 2 * ne);
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const int64_t n = (int64_t)ids.size();
    auto dense = [&](int64_t g) { return (int64_t)(std::lower_bound(ids.begin(), ids.end(), g) - ids.begin()); };
    std::vector<std::pair<int64_t, int64_t>> ed;
    ed.reserve((size_t)ne * 2);
    for (int64_t k = 0; k < ne; ++k) {
        const int64_t a = dense(edges[2 * k]), b = dense(edges[2 * k + 1]);
        ed.emplace_back(a, b);
        ed.emplace_back(b, a);
    }
    std::sort(ed.begin(), ed.end());
    ed.erase(std::unique(ed.begin(), ed.end()), ed.end());
    std::vector<int64_t> off((size_t)n + 1, 0), nb(ed.size());
    for (const auto& p : ed) ++off[(size_t)p.first + 1];
    for (int64_t i = 0; i < n; ++i) off[(size_t)i + 1] += off[(size_t)i];
    for (size_t k = 0; k < ed.size(); ++k) nb[k] = ed[k].second;
    // _rims_touching (:67-95): whole components holding a seed (every component without seeds)
    std::vector<int64_t> comp((size_t)n, -1);
    std::vector<uint8_t> keep_comp;
    std::vector<int64_t> stack;
    for (int64_t s = 0; s < n; ++s) {
        if (comp[(size_t)s] >= 0) continue;
        const int64_t c = (int64_t)keep_comp.size();
        bool seeded = !have_seeds;
        comp[(size_t)s] = c;
        stack.assign(1, s);
        while (!stack.empty()) {
            const int64_t x = stack.back();
            stack.pop_back();
            if (!seeded && std::binary_search(seeds.begin(), seeds.end(), ids[(size_t)x])) seeded = true;
            for (int64_t k = off[(size_t)x]; k < off[(size_t)x + 1]; ++k)
                if (comp[(size_t)nb[(size_t)k]] < 0) { comp[(size_t)nb[(size_t)k]] = c; stack.push_back(nb[(size_t)k]); }
        }
        keep_comp.push_back(seeded ? 1 : 0);
    }
    std::vector<uint8_t> remaining((size_t)n, 0);
    bool any = false;
    for (int64_t i = 0; i < n; ++i)
        if (keep_comp[(size_t)comp[(size_t)i]]) { remaining[(size_t)i] = 1; any = true; out.rim.push_back(ids[(size_t)i]); }
    if (clean) {
        if (!any) return;
        for (int64_t i = 0; i < n; ++i)                                                   // :306-311
            if (remaining[(size_t)i] && off[(size_t)i + 1] - off[(size_t)i] != 2) out.drop.push_back(ids[(size_t)i]);
        if (!out.drop.empty()) return;
    }
    // _walk_rings (:98-118) with the fixed rule
    std::vector<Ring> rings;
    for (int64_t s = 0; s < n; ++s) {
        if (!remaining[(size_t)s]) continue;
        Ring ring(1, ids[(size_t)s]);
        remaining[(size_t)s] = 0;
        int64_t prev = -1, cur = s;
        for (;;) {
            int64_t nxt = -1;
            for (int64_t k = off[(size_t)cur]; k < off[(size_t)cur + 1]; ++k) {
                const int64_t w = nb[(size_t)k];
                if (w != prev && remaining[(size_t)w]) { nxt = w; break; }
            }
            if (nxt < 0) break;
            ring.push_back(ids[(size_t)nxt]);
            remaining[(size_t)nxt] = 0;
            prev = cur;
            cur = nxt;
        }
        rings.push_back(std::move(ring));
    }
    if (clean) {                                                                          // :313-321
        for (const Ring& r : rings) {
            Ring kept = despike(r, v, despike_cos);
            std::sort(kept.begin(), kept.end());
            for (int64_t x : r)
                if (!std::binary_search(kept.begin(), kept.end(), x)) out.drop.push_back(x);
        }
        if (!out.drop.empty()) {
            std::sort(out.drop.begin(), out.drop.end());
            return;
        }
    }
    out.rings = reduce_rings(std::move(rings), v, target_n);
}

// ---- device part -----------------------------------------------------------------------------------------------------

// The device buffers of one trim, carved out of the engine's grow-only device buffer.  The hash table has the slots of
// the edge table (EdgeTable::log2_slots) without the owner plane: 12 bytes a slot.
struct TrimDev {
    int32_t* face = nullptr;
    double* vert = nullptr;
    uint8_t *in = nullptr, *fk = nullptr, *mark = nullptr;
    unsigned long long *keys = nullptr, *open = nullptr, *n_open = nullptr;
    unsigned int* cnt = nullptr;
    int32_t *vidx = nullptr, *fidx = nullptr, *drop = nullptr, *out_f = nullptr;
    long long *vtile = nullptr, *ftile = nullptr;
    double* out_v = nullptr;
    int log2_cap = 8;
};

// Device layout for nv vertices and nf faces (vertices only where with_vertices); the faces, converted to int32, and
// the vertices (with_vertices) go up in one copy from the pinned buffer, which is left sized for every download.
int trim_alloc(Engine* e, const double* v, int64_t nv, const int64_t* faces, int64_t nf, bool with_vertices, TrimDev& d)
{
    d.log2_cap = EdgeTable::log2_slots(nf);
    const size_t cap = (size_t)1 << d.log2_cap, V = (size_t)nv, Fn = (size_t)nf, vert_n = with_vertices ? 3 * V : 0;
    size_t o_vert = 0, in_bytes = 0;
    int rc = carve_on(e, e->dev_pts, [&](Carve& c) {
        c.place(d.face, 3 * Fn); o_vert = c.place(d.vert, vert_n);
        in_bytes = c.size();
        c.place(d.in, V); c.place(d.fk, Fn); c.place(d.mark, V);
        c.place(d.keys, cap); c.place(d.cnt, cap);
        c.place(d.open, 3 * Fn); c.place(d.n_open, 1);
        c.place(d.vidx, V); c.place(d.fidx, Fn); c.place(d.drop, V);
        c.place(d.vtile, trim_scan_tiles(nv) + 1); c.place(d.ftile, trim_scan_tiles(nf) + 1);
        c.place(d.out_v, vert_n); c.place(d.out_f, 3 * Fn);
    });
    if (rc) return rc;
    const size_t host_bytes = std::max({in_bytes, Fn * 24, V * 24 + Fn * 12, V + 256});
    if ((rc = e->ensure(e->host_pts, host_bytes, true))) return rc;
    unsigned char* h = (unsigned char*)e->host_pts.p;
    narrow_faces((int32_t*)h, faces, 3 * nf);
    if (with_vertices && nv > 0) std::memcpy(h + o_vert, v, V * 24);
    if (in_bytes) MM_TRY_HIP(hipMemcpyAsync(d.face, h, in_bytes, hipMemcpyHostToDevice, e->stream));
    return MM_OK;
}

// faces surviving the vertex mask d.in (all corners in it) -> d.fk, and their open edges, sorted, as (a, b) pairs
int open_edges_now(Engine* e, TrimDev& d, int64_t nf, std::vector<int64_t>& edges)
{
    MM_TRY_HIP(launch_trim_faces(d.face, nf, d.in, 0, d.fk, nullptr, e->stream));
    MM_TRY_HIP(launch_trim_open_edges(d.face, nf, d.fk, d.keys, d.cnt, d.log2_cap, d.open, d.n_open, e->stream));
    unsigned long long* h = (unsigned long long*)e->host_pts.p;
    MM_TRY_HIP(hipMemcpyAsync(h, d.n_open, 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    const unsigned long long n = h[0];
    if (n > (unsigned long long)nf * 3) return set_error(MM_ERR_HIP, "open boundary edges: count out of range");
    if (n) {
        MM_TRY_HIP(hipMemcpyAsync(h, d.open, n * 8, hipMemcpyDeviceToHost, e->stream));
        MM_TRY_HIP(hipStreamSynchronize(e->stream));
    }
    std::sort(h, h + n);
    edges.resize(2 * n);
    for (unsigned long long k = 0; k < n; ++k) { edges[2 * k] = (int64_t)(h[k] >> 32); edges[2 * k + 1] = (int64_t)(h[k] & 0xFFFFFFFFull); }
    return MM_OK;
}

// clean_open_boundary (boundary.py:257-325) on the faces that survive d.in: every round re-derives the surviving faces
// and their open edges on the device; the vertices it culls are cleared in d.in and added to `dropped`
int clean_loop(Engine* e, TrimDev& d, int64_t nf, const double* v, std::vector<int64_t> seeds, bool have_seeds,
               int64_t target_n, double despike_cos, int64_t max_rounds, std::vector<int64_t>& dropped,
               std::vector<Ring>& rings)
{
    std::sort(seeds.begin(), seeds.end());
    seeds.erase(std::unique(seeds.begin(), seeds.end()), seeds.end());
    std::vector<int64_t> edges;
    RimResult rr;
    int rc;
    for (int64_t round = 0; round < max_rounds; ++round) {
        if ((rc = open_edges_now(e, d, nf, edges))) return rc;
        rim_pass(edges.data(), (int64_t)edges.size() / 2, seeds, have_seeds, v, target_n, despike_cos, true, rr);
        if (rr.rim.empty()) { rings.clear(); return MM_OK; }                                         // :300-301
        std::vector<int64_t> grown;                                                                   // :304
        std::set_union(seeds.begin(), seeds.end(), rr.rim.begin(), rr.rim.end(), std::back_inserter(grown));
        seeds.swap(grown);
        have_seeds = true;
        if (rr.drop.empty()) { rings = std::move(rr.rings); return MM_OK; }
        std::vector<int64_t> all;
        std::set_union(dropped.begin(), dropped.end(), rr.drop.begin(), rr.drop.end(), std::back_inserter(all));
        dropped.swap(all);
        int32_t* h = (int32_t*)e->host_pts.p;
        for (size_t k = 0; k < rr.drop.size(); ++k) h[k] = (int32_t)rr.drop[k];
        MM_TRY_HIP(hipMemcpyAsync(d.drop, h, rr.drop.size() * 4, hipMemcpyHostToDevice, e->stream));
        MM_TRY_HIP(launch_trim_clear(d.drop, (long long)rr.drop.size(), d.in, e->stream));
        MM_TRY_HIP(hipStreamSynchronize(e->stream));                    // the pinned buffer is reused next round
    }
    if ((rc = open_edges_now(e, d, nf, edges))) return rc;                                            // :323-325
    rim_pass(edges.data(), (int64_t)edges.size() / 2, seeds, have_seeds, v, target_n, despike_cos, false, rr);
    rings = std::move(rr.rings);
    return MM_OK;
}

int write_rings(const std::vector<Ring>& rings, int64_t* ring_len, int64_t* ring_idx, int64_t* n_rings, int64_t* n_idx)
{
    int64_t k = 0;
    for (size_t r = 0; r < rings.size(); ++r) {
        ring_len[r] = (int64_t)rings[r].size();
        std::copy(rings[r].begin(), rings[r].end(), ring_idx + k);
        k += (int64_t)rings[r].size();
    }
    *n_rings = (int64_t)rings.size();
    *n_idx = k;
    return MM_OK;
}

}  // namespace
}  // namespace mm

using namespace mm;

extern "C" {

int mm_boundary_rings(const int64_t* edges, int64_t ne, const int64_t* seeds, int64_t ns, const double* vertices_xyz,
                      int64_t nv, int64_t target_n, double despike_cos, int clean, int64_t* ring_len, int64_t* ring_idx,
                      int64_t* drop, int64_t* rim, int64_t* counts)
{
    if (ne < 0 || ns < 0 || nv < 0 || nv > kMaxIndex || !counts || (ne > 0 && (!edges || !vertices_xyz || !ring_len ||
        !ring_idx)) || (ns > 0 && !seeds) || (clean && ne > 0 && (!drop || !rim)) || (target_n < 1 && target_n != -1) ||
        (clean != 0 && clean != 1))
        return set_error(MM_ERR_INVALID, "mm_boundary_rings: bad arguments");
    for (int64_t k = 0; k < 2 * ne; ++k)
        if (edges[k] < 0 || edges[k] >= nv) return set_error(MM_ERR_INVALID, "mm_boundary_rings: edge end out of range");
    std::vector<int64_t> s(seeds, seeds + ns);
    std::sort(s.begin(), s.end());
    RimResult rr;
    rim_pass(edges, ne, s, ns > 0, vertices_xyz, target_n, despike_cos, clean != 0, rr);
    write_rings(rr.rings, ring_len, ring_idx, counts, counts + 1);
    counts[2] = (int64_t)rr.drop.size();
    counts[3] = (int64_t)rr.rim.size();
    if (clean) {
        std::copy(rr.drop.begin(), rr.drop.end(), drop);
        std::copy(rr.rim.begin(), rr.rim.end(), rim);
    }
    return MM_OK;
}

int mm_build_adjacency(const int64_t* faces, int64_t nf, int64_t nv, int64_t* off, int64_t* nb)
{
    if (nf < 0 || nv < 0 || (nf > 0 && (!faces || !nb)) || !off)
        return set_error(MM_ERR_INVALID, "mm_build_adjacency: bad arguments");
    if (const int rc = faces_in_range(faces, nf, nv, "mm_build_adjacency")) return rc;
    Adjacency adj;
    build_adjacency(faces, nf, nv, adj);
    std::copy(adj.off.begin(), adj.off.end(), off);
    std::copy(adj.nb.begin(), adj.nb.end(), nb);
    return MM_OK;
}

int64_t mm_open_boundary_edges(mm_engine* h, const int64_t* faces, int64_t nf, int64_t nv, int64_t* edges)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (nf < 0 || nv < 0 || nf > kMaxIndex || nv > kMaxIndex || (nf > 0 && (!faces || !edges)))
        return set_error(MM_ERR_INVALID, "mm_open_boundary_edges: bad arguments");
    if ((rc = faces_in_range(faces, nf, nv, "mm_open_boundary_edges"))) return rc;
    if (nf == 0) return 0;
    TrimDev d;
    if ((rc = trim_alloc(e, nullptr, nv, faces, nf, false, d))) return rc;
    MM_TRY_HIP(hipMemsetAsync(d.in, 1, (size_t)nv, e->stream));
    std::vector<int64_t> ed;
    if ((rc = open_edges_now(e, d, nf, ed))) return rc;
    std::copy(ed.begin(), ed.end(), edges);
    return (int64_t)ed.size() / 2;
}

int mm_clean_open_boundary(mm_engine* h, const int64_t* faces, int64_t nf, const double* vertices_xyz, int64_t nv,
                           const int64_t* seeds, int64_t ns, int64_t target_n, double despike_cos, int64_t max_rounds,
                           int64_t* drop, int64_t* ring_len, int64_t* ring_idx, int64_t* counts)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (nf < 0 || nv < 0 || ns < 0 || nf > kMaxIndex || nv > kMaxIndex || !counts || (nf > 0 && !faces) ||
        (nv > 0 && (!vertices_xyz || !drop || !ring_len || !ring_idx)) || (ns > 0 && !seeds) ||
        (target_n < 1 && target_n != -1))
        return set_error(MM_ERR_INVALID, "mm_clean_open_boundary: bad arguments");
    if ((rc = faces_in_range(faces, nf, nv, "mm_clean_open_boundary"))) return rc;
    std::memset(counts, 0, 3 * sizeof(int64_t));
    if (nf == 0) return MM_OK;                         // no open edge: no rim, nothing dropped
    TrimDev d;
    if ((rc = trim_alloc(e, nullptr, nv, faces, nf, false, d))) return rc;
    MM_TRY_HIP(hipMemsetAsync(d.in, 1, (size_t)nv, e->stream));
    std::vector<int64_t> dropped;
    std::vector<Ring> rings;
    if ((rc = clean_loop(e, d, nf, vertices_xyz, std::vector<int64_t>(seeds, seeds + ns), ns > 0, target_n, despike_cos,
                         max_rounds, dropped, rings)))
        return rc;
    std::copy(dropped.begin(), dropped.end(), drop);
    counts[2] = (int64_t)dropped.size();
    return write_rings(rings, ring_len, ring_idx, counts, counts + 1);
}

int mm_trim_mesh(mm_engine* h, const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf,
                 const uint8_t* region, int mode, int64_t target_n, double despike_cos, int64_t max_rounds,
                 double* out_vertices, int64_t* out_faces, int64_t* ring_len, int64_t* ring_idx, int64_t* counts)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (nf < 0 || nv < 0 || nf > kMaxIndex || nv > kMaxIndex || !counts || (mode != 0 && mode != 1 && mode != 2) ||
        (nf > 0 && (!faces || !out_faces)) || (nv > 0 && (!vertices_xyz || !region || !out_vertices)) ||
        (mode != 2 && nv > 0 && (!ring_len || !ring_idx)) || (target_n < 1 && target_n != -1))
        return set_error(MM_ERR_INVALID, "mm_trim_mesh: bad arguments");
    if ((rc = faces_in_range(faces, nf, nv, "mm_trim_mesh"))) return rc;
    std::memset(counts, 0, 4 * sizeof(int64_t));
    if (nv == 0) return MM_OK;
    TrimDev d;
    if ((rc = trim_alloc(e, vertices_xyz, nv, faces, nf, true, d))) return rc;
    uint8_t* hm = (uint8_t*)e->host_pts.p;
    MM_TRY_HIP(hipStreamSynchronize(e->stream));                        // the mesh upload has left the pinned buffer
    for (int64_t i = 0; i < nv; ++i) hm[i] = mode == 0 ? (region[i] ? 0 : 1) : (region[i] ? 1 : 0);
    MM_TRY_HIP(hipMemcpyAsync(d.in, hm, (size_t)nv, hipMemcpyHostToDevice, e->stream));
    MM_TRY_HIP(hipMemsetAsync(d.mark, 0, (size_t)nv, e->stream));
    const uint8_t* vmask = d.in;
    std::vector<Ring> rings;
    if (mode == 2) {                                     // _extract_region_with_border_faces: faces touching the region
        MM_TRY_HIP(launch_trim_faces(d.face, nf, d.in, 1, d.fk, d.mark, e->stream));
        vmask = d.mark;                                  // its used vertices only
    } else {                                             // remove / keep: rim seeds, then the cleaning rounds
        MM_TRY_HIP(launch_trim_faces(d.face, nf, d.in, 0, d.fk, d.mark, e->stream));
        MM_TRY_HIP(hipMemcpyAsync(hm, d.mark, (size_t)nv, hipMemcpyDeviceToHost, e->stream));
        MM_TRY_HIP(hipStreamSynchronize(e->stream));
        std::vector<int64_t> seeds;
        for (int64_t i = 0; i < nv; ++i)
            if (hm[i]) seeds.push_back(i);
        std::vector<int64_t> dropped;
        const bool have = !seeds.empty();
        if ((rc = clean_loop(e, d, nf, vertices_xyz, std::move(seeds), have, target_n, despike_cos, max_rounds, dropped,
                             rings)))
            return rc;
    }
    MM_TRY_HIP(launch_trim_scan(vmask, nv, d.vtile, d.vidx, e->stream));
    MM_TRY_HIP(launch_trim_scan(d.fk, nf, d.ftile, d.fidx, e->stream));
    MM_TRY_HIP(launch_trim_compact(d.vert, nv, d.vidx, d.face, nf, d.fidx, d.out_v, d.out_f, e->stream));
    long long kv, kf;
    if ((rc = scan_totals(e, d.vtile, nv, d.ftile, nf, &kv, &kf, "mm_trim_mesh"))) return rc;
    unsigned char* hb = (unsigned char*)e->host_pts.p;
    if (kv) MM_TRY_HIP(hipMemcpyAsync(hb, d.out_v, (size_t)kv * 24, hipMemcpyDeviceToHost, e->stream));
    if (kf) MM_TRY_HIP(hipMemcpyAsync(hb + (size_t)kv * 24, d.out_f, (size_t)kf * 12, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    std::memcpy(out_vertices, hb, (size_t)kv * 24);
    const int32_t* f32 = (const int32_t*)(hb + (size_t)kv * 24);
    widen_faces(out_faces, f32, 3 * kf);
    counts[0] = kv;
    counts[1] = kf;
    return write_rings(rings, ring_len, ring_idx, counts + 2, counts + 3);
}

}  // extern "C"
