// mm_geodesic.cpp -- a centerline from a mesh (include/mm_centerline.h, rules G, S and T): the geodesic
// distance field over the edge graph, the band skeleton, and the tree of branches.  The reference has no counterpart:
// "Create Centerline directly from mesh" is an open item of its roadmap.
//
// Field and skeleton run on the device (mm_geodesic_kernels.hip; the edge table and the jumping round of
// mm_weld_kernels.hip, the sorted adjacency, the row scan and the row sort of mm_smooth_kernels.hip, the flag scan of
// mm_trim_kernels.hip).  The host checks the arguments, narrows faces and seeds to int32, uploads once, launches the
// field's rounds in batches and reads one small record of marks back per batch; the skeleton reads a word per jumping
// round and the two counts (nodes, node edges) that size its sorts and its output; the results come down in one go.
// mm_skeleton_centerline is host code over thousands of nodes at most.
//
// The upload, [vertices | faces | seeds], lives in e->dev_pts and is never written.  The rest is carved from e->dev_raw:
// the adjacency (CsrDev of mm_stage.h), one weight per adjacency entry, the seed bytes, the two flag arrays, the marks
// of a batch, [dist | pred | counters] and, for the skeleton, what SkelScratch lists (mm_mesh_layout.h).
#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/mm_centerline.h"
#include "mm_mesh_layout.h"

namespace mm {

void cl_recompute_tangents(mm_clpoint* p, int64_t n);                  // mm_cl_branches.cpp

namespace {

constexpr int kFirstBatch = 8, kLongestBatch = 64;     // rounds between two reads of the marks

// The field, staged and computed: everything stays on the device.  reserve() -> run().  The device buffers are those
// of FieldScratch (mm_mesh_layout.h).
struct Field : FieldScratch {
    Engine* e = nullptr;
    int64_t nv = 0, nf = 0, n_seeds = 0;
    size_t u_v = 0, u_f = 0, u_s = 0, up_bytes = 0;                    // the upload: the same offsets on host and device
    unsigned char *hb = nullptr, *b = nullptr;
    const double* v = nullptr;
    const int32_t *face = nullptr, *seeds = nullptr;
    int launches = 0;
    int64_t mark_bytes = 0;

    // behind: what the caller downloads behind the field's block, from up256(field_down()) on
    int reserve(Engine* engine, int64_t nv_, int64_t nf_, int64_t ns, bool skeleton, size_t behind)
    {
        e = engine;
        nv = nv_; nf = nf_; n_seeds = ns;
        int rc = carve_on(e, e->dev_pts, [&](Carve& c) {
            u_v = c.place(v, 3 * (size_t)nv); u_f = c.place(face, 3 * (size_t)nf); u_s = c.place(seeds, (size_t)ns);
            up_bytes = c.size();
        });
        if (rc) return rc;
        if ((rc = carve_on(e, e->dev_raw, [&](Carve& c) { lay(c, nv, nf, kLongestBatch, skeleton); }))) return rc;
        const size_t down = behind ? up256(field_down()) + behind : field_down();
        if ((rc = e->ensure(e->host_pts, std::max(up_bytes, down) + 512, true))) return rc;
        hb = (unsigned char*)e->host_pts.p;
        b = (unsigned char*)e->dev_pts.p;
        d.counts = counts + geo_num_csr;
        return MM_OK;
    }

    // upload, adjacency, weights, the rounds, the predecessors; rep takes rounds and n_batches
    int run(const double* vertices_xyz, const int64_t* faces, const int64_t* seed_idx, mm_geodesic_report& rep, const char* who)
    {
        std::memcpy(hb + u_v, vertices_xyz, (size_t)nv * 24);
        narrow_faces((int32_t*)(hb + u_f), faces, 3 * nf);
        narrow_faces((int32_t*)(hb + u_s), seed_idx, n_seeds);
        MM_TRY_HIP(hipMemcpyAsync(b, hb, up_bytes, hipMemcpyHostToDevice, e->stream));
        unsigned int *cur = flag_a, *next = flag_b;
        MM_TRY_HIP(hipMemsetAsync(counts, 0, geo_num_words * 8, e->stream));
        if (const int rc = csr_build(e, d, face, nf, nv, &launches)) return rc;
        MM_TRY_HIP(launch_geo_weights(v, d.off, d.nb, nv, w, counts, e->stream));
        MM_TRY_HIP(launch_geo_seed(seeds, n_seeds, d.off, d.nb, nv, dist, is_seed, cur, next, e->stream));
        launches += 3;

        // rounds until one raises no flag.  A vertex whose shortest path has k edges is final after round k (its
        // predecessor's owner flagged its block when the predecessor fell for the last time), so nv rounds always do.
        unsigned long long* hm = (unsigned long long*)hb;
        int batch = kFirstBatch;
        for (bool settled = false; !settled;) {
            MM_TRY_HIP(hipMemsetAsync(marks, 0, (size_t)batch * 8, e->stream));
            for (int k = 0; k < batch; ++k) {
                MM_TRY_HIP(launch_geo_round(d.off, d.nb, w, nv, dist, cur, next, marks + k, e->stream));
                std::swap(cur, next);
            }
            MM_TRY_HIP(hipMemcpyAsync(hm, marks, (size_t)batch * 8, hipMemcpyDeviceToHost, e->stream));
            MM_TRY_HIP(hipStreamSynchronize(e->stream));
            launches += batch;
            mark_bytes += (int64_t)batch * 8;
            ++rep.n_batches;
            int ran = batch;
            for (int k = 0; k < batch; ++k)
                if (hm[k] == 0) {                                       // the rounds behind it found no flag
                    ran = k + 1;
                    settled = true;
                    break;
                }
            rep.rounds += ran;
            if (!settled && rep.rounds > nv + 1) return set_error(MM_ERR_HIP, std::string(who) + ": the field did not settle");
            batch = std::min(2 * batch, kLongestBatch);
        }
        MM_TRY_HIP(launch_geo_pred(d.off, d.nb, w, dist, is_seed, nv, pred, counts, e->stream));
        ++launches;
        return MM_OK;
    }

    // [dist | pred | counters] as downloaded to `from` -> the caller's arrays and the report
    int finish(const unsigned char* from, double* out_dist, int64_t* out_pred, mm_geodesic_report& rep, const char* who) const
    {
        std::memcpy(out_dist, from, (size_t)nv * 8);
        const int32_t* hp = (const int32_t*)(from + (o_pred - o_dist));
        for (int64_t i = 0; i < nv; ++i) out_pred[i] = hp[i];
        const unsigned long long* hc = (const unsigned long long*)(from + (o_counts - o_dist));
        const int64_t all_edges = (int64_t)hc[geo_num_csr];
        if (all_edges < 0 || all_edges > 3 * nf || (int64_t)hc[geo_num_skipped] > all_edges || (int64_t)hc[geo_num_reached] > nv)
            return set_error(MM_ERR_HIP, std::string(who) + ": a count is out of range");
        rep.n_skipped_edges = (int64_t)hc[geo_num_skipped];
        rep.n_edges = all_edges - rep.n_skipped_edges;
        rep.n_reached = (int64_t)hc[geo_num_reached];
        std::memcpy(&rep.max_dist, &hc[geo_num_max_dist], 8);
        std::memcpy(&rep.max_edge, &hc[geo_num_max_edge], 8);
        rep.n_launches = launches;
        rep.bytes_uploaded = (int64_t)((size_t)nv * 24 + (size_t)nf * 12 + (size_t)n_seeds * 4);
        rep.bytes_downloaded = (int64_t)((size_t)nv * 12 + geo_num_words * 8) + mark_bytes;
        return MM_OK;
    }
};

// the checks the two device entry points share
int field_args(const char* who, const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf, const int64_t* seeds,
               int64_t n_seeds, const double* dist, const int64_t* pred)
{
    if (n_seeds <= 0 || n_seeds > kMaxIndex || !seeds || (nv > 0 && (!dist || !pred)))
        return set_error(MM_ERR_INVALID, std::string(who) + ": bad arguments");
    if (const int rc = mesh_args(who, vertices_xyz, nv, faces, nf, true)) return rc;
    for (int64_t k = 0; k < n_seeds; ++k)
        if (seeds[k] < 0 || seeds[k] >= nv) return set_error(MM_ERR_INVALID, std::string(who) + ": seed out of range");
    return MM_OK;
}

inline double gap(const double* a, const double* b)
{
    const double dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
    return std::sqrt((dx * dx + dy * dy) + dz * dz);
}

}  // namespace
}  // namespace mm

using namespace mm;

extern "C" {

int mm_mesh_geodesic(mm_engine* h, const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf,
                     const int64_t* seeds, int64_t n_seeds, double* dist, int64_t* pred, mm_geodesic_report* report)
{
    static const char* who = "mm_mesh_geodesic";
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (!report) return set_error(MM_ERR_INVALID, std::string(who) + ": bad arguments");
    if ((rc = field_args(who, vertices_xyz, nv, faces, nf, seeds, n_seeds, dist, pred))) return rc;
    mm_geodesic_report rep;
    std::memset(&rep, 0, sizeof(rep));
    rep.n_vertices = nv;
    rep.n_faces = nf;
    Field fd;
    if ((rc = fd.reserve(e, nv, nf, n_seeds, false, 0))) return rc;
    if ((rc = fd.run(vertices_xyz, faces, seeds, rep, who))) return rc;
    MM_TRY_HIP(hipMemcpyAsync(fd.hb, fd.dist, fd.field_down(), hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    if ((rc = fd.finish(fd.hb, dist, pred, rep, who))) return rc;
    *report = rep;
    return MM_OK;
}

int mm_mesh_skeleton(mm_engine* h, const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf,
                     const int64_t* seeds, int64_t n_seeds, double band_mm, int64_t node_cap, int64_t edge_cap, double* dist,
                     int64_t* pred, int64_t* vertex_node, mm_skeleton_node* nodes, int64_t* edges,
                     mm_skeleton_report* report)
{
    static const char* who = "mm_mesh_skeleton";
    static_assert(sizeof(mm_skeleton_node) == 80, "the kernel writes ten words a node");
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (!report || !std::isfinite(band_mm) || !(band_mm > 0.0) || node_cap < 0 || edge_cap < 0 ||
        (nv > 0 && !vertex_node) || (node_cap > 0 && !nodes) || (edge_cap > 0 && !edges))
        return set_error(MM_ERR_INVALID, std::string(who) + ": bad arguments");
    if ((rc = field_args(who, vertices_xyz, nv, faces, nf, seeds, n_seeds, dist, pred))) return rc;
    mm_skeleton_report rep;
    std::memset(&rep, 0, sizeof(rep));
    rep.field.n_vertices = nv;
    rep.field.n_faces = nf;
    rep.band_mm = band_mm;
    Field fd;
    // the host side of the download: the field's block, vertex_node, the nodes, the edges
    const size_t behind = up256((size_t)nv * 4) + up256((size_t)nv * 80) + 3 * (size_t)nf * 8;
    if ((rc = fd.reserve(e, nv, nf, n_seeds, true, behind))) return rc;
    const size_t h_vnode = up256(fd.field_down()), h_rec = h_vnode + up256((size_t)nv * 4), h_edges = h_rec + up256((size_t)nv * 80);
    if ((rc = fd.run(vertices_xyz, faces, seeds, rep.field, who))) return rc;

    const SkelScratch& sk = fd.sk;
    int launches = fd.launches;

    // bands and their components
    MM_TRY_HIP(launch_skel_bands(fd.dist, nv, band_mm, fd.d.off, fd.d.nb, fd.w, sk.band, sk.link, fd.counts, e->stream));
    launches += 2;
    unsigned int* hc = (unsigned int*)fd.hb;
    const int64_t bound = 2 + log2_at_least((unsigned long long)nv) + 8;   // a jumping round halves the depth
    for (;;) {
        MM_TRY_HIP(launch_weld_jump(sk.link, nv, sk.changed, e->stream));
        MM_TRY_HIP(hipMemcpyAsync(hc, sk.changed, 4, hipMemcpyDeviceToHost, e->stream));
        MM_TRY_HIP(hipStreamSynchronize(e->stream));
        ++rep.union_rounds;
        if (!hc[0]) break;
        if (rep.union_rounds > bound) return set_error(MM_ERR_HIP, std::string(who) + ": pointer jumping did not settle");
    }
    launches += (int)rep.union_rounds;
    MM_TRY_HIP(launch_skel_roots(sk.link, sk.band, nv, sk.is_root, e->stream));
    MM_TRY_HIP(launch_trim_scan(sk.is_root, nv, sk.rtile, sk.ridx, e->stream));
    launches += 4;
    unsigned long long* hn = (unsigned long long*)fd.hb;
    MM_TRY_HIP(hipMemcpyAsync(hn, sk.rtile + trim_scan_tiles(nv), 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(hn + 1, fd.counts + geo_num_band_over, 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    if (hn[1]) return set_error(MM_ERR_TOO_LARGE, std::string(who) + ": a band index passes 2^31");
    const int64_t K = (int64_t)hn[0];
    if (K < 1 || K > nv) return set_error(MM_ERR_HIP, std::string(who) + ": node count out of range");

    // numbered by (band, smallest vertex); the lists of every node in order; the records
    MM_TRY_HIP(launch_skel_keys(sk.ridx, sk.band, nv, K, sk.sortbuf, e->stream));
    ++launches;
    MM_TRY_HIP(launch_geo_sort(sk.sortbuf, K, &launches, e->stream));
    MM_TRY_HIP(launch_skel_number(sk.sortbuf, K, sk.ridx, fd.d.edges.keys, fd.d.edges.cnt, fd.d.edges.log2_e, sk.link, sk.band, fd.is_seed,
                                  nv, sk.rim, sk.vnode, sk.nflags, sk.vcnt, sk.ccnt, e->stream));
    MM_TRY_HIP(launch_skel_faces(fd.v, fd.face, nf, sk.vnode, sk.area3, sk.ccnt, e->stream));
    launches += 3 + (nf > 0);
    MM_TRY_HIP(hipMemsetAsync(sk.scan_counts, 0, 4 * 8, e->stream));
    MM_TRY_HIP(launch_mesh_row_offsets(sk.vcnt, K, sk.voff, sk.tile, sk.scan_counts, &launches, e->stream));
    MM_TRY_HIP(launch_mesh_row_offsets(sk.ccnt, K, sk.coff, sk.tile, sk.scan_counts, &launches, e->stream));
    MM_TRY_HIP(launch_skel_fill(fd.face, nf, sk.vnode, nv, sk.ccnt, sk.clist, sk.vcnt, sk.vlist, e->stream));
    ++launches;
    MM_TRY_HIP(launch_mesh_row_sort(sk.voff, sk.vlist, K, &launches, e->stream));
    MM_TRY_HIP(launch_mesh_row_sort(sk.coff, sk.clist, K, &launches, e->stream));
    MM_TRY_HIP(launch_skel_nodes(K, sk.coff, sk.clist, sk.voff, sk.vlist, fd.face, sk.area3, fd.v, sk.band, sk.nflags, sk.rec, e->stream));
    ++launches;

    // the node edges: the edge table's keys are free once the rim is marked
    MM_TRY_HIP(launch_skel_edges(fd.d.off, fd.d.nb, fd.w, sk.vnode, nv, fd.d.edges.keys, fd.d.edges.log2_e, sk.sortbuf, sk.n_out, e->stream));
    launches += 2;
    MM_TRY_HIP(hipMemcpyAsync(hn, sk.n_out, 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    const int64_t M = (int64_t)hn[0];
    if (M < 0 || M > 3 * nf) return set_error(MM_ERR_HIP, std::string(who) + ": node edge count out of range");
    rep.n_nodes = K;
    rep.n_node_edges = M;
    if (K > node_cap || M > edge_cap) {
        *report = rep;
        return set_error(MM_ERR_TOO_LARGE, std::string(who) + ": node_cap or edge_cap too small (the report holds the sizes)");
    }
    MM_TRY_HIP(launch_geo_sort(sk.sortbuf, M, &launches, e->stream));

    unsigned char* hb = fd.hb;
    MM_TRY_HIP(hipMemcpyAsync(hb, fd.dist, fd.field_down(), hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(hb + h_vnode, sk.vnode, (size_t)nv * 4, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(hb + h_rec, sk.rec, (size_t)K * 80, hipMemcpyDeviceToHost, e->stream));
    if (M > 0) MM_TRY_HIP(hipMemcpyAsync(hb + h_edges, sk.sortbuf, (size_t)M * 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    fd.launches = launches;
    if ((rc = fd.finish(hb, dist, pred, rep.field, who))) return rc;
    const int32_t* hv = (const int32_t*)(hb + h_vnode);
    for (int64_t i = 0; i < nv; ++i) vertex_node[i] = hv[i];
    std::memcpy(nodes, hb + h_rec, (size_t)K * 80);
    const unsigned long long* he = (const unsigned long long*)(hb + h_edges);
    for (int64_t k = 0; k < M; ++k) {
        edges[2 * k] = (int64_t)(he[k] >> 32);
        edges[2 * k + 1] = (int64_t)(he[k] & 0xFFFFFFFFull);
    }
    rep.n_launches = launches;
    rep.bytes_uploaded = rep.field.bytes_uploaded;
    rep.bytes_downloaded = rep.field.bytes_downloaded + (int64_t)((size_t)nv * 4 + (size_t)K * 80 + (size_t)M * 8) +
                           4 * rep.union_rounds + 24;
    *report = rep;
    return MM_OK;
}

int64_t mm_skeleton_centerline(const mm_skeleton_node* nodes, int64_t n_nodes, const int64_t* edges, int64_t n_edges,
                               const mm_skeleton_terminal* terminals, int64_t n_terminals, double min_branch_mm,
                               mm_clpoint* out, int64_t* point_node, int64_t* branch_info, int64_t cap,
                               mm_tree_report* report)
{
    static const char* who = "mm_skeleton_centerline";
    const int64_t K = n_nodes, T = n_terminals, A = K + T;
    if (!report || K < 0 || n_edges < 0 || T < 0 || K > kMaxIndex || T > kMaxIndex || n_edges > kMaxIndex || cap < A ||
        std::isnan(min_branch_mm) || (K > 0 && !nodes) || (n_edges > 0 && !edges) || (T > 0 && !terminals) ||
        (A > 0 && (!out || !point_node || !branch_info)))
        return set_error(MM_ERR_INVALID, std::string(who) + ": bad arguments");
    for (int64_t n = 1; n < K; ++n)
        if (nodes[n].band < nodes[n - 1].band) return set_error(MM_ERR_INVALID, std::string(who) + ": nodes are not in band order");
    for (int64_t k = 0; k < n_edges; ++k)
        if (edges[2 * k] < 0 || edges[2 * k] >= edges[2 * k + 1] || edges[2 * k + 1] >= K)
            return set_error(MM_ERR_INVALID, std::string(who) + ": a node edge is not lo < hi inside the nodes");
    for (int64_t j = 0; j < T; ++j)
        if (terminals[j].node < 0 || terminals[j].node >= K)
            return set_error(MM_ERR_INVALID, std::string(who) + ": a terminal's node is out of range");
    mm_tree_report rep;
    std::memset(&rep, 0, sizeof(rep));
    rep.n_terminals = T;

    // parents: the adjacent node of lower band with the smallest number; components and loops
    std::vector<std::vector<int64_t>> adj((size_t)K);
    std::vector<int64_t> comp((size_t)K);
    for (int64_t n = 0; n < K; ++n) comp[n] = n;
    auto find = [&](int64_t x) { while (comp[x] != x) x = comp[x] = comp[comp[x]]; return x; };
    for (int64_t k = 0; k < n_edges; ++k) {
        const int64_t a = edges[2 * k], b = edges[2 * k + 1];
        adj[a].push_back(b);
        adj[b].push_back(a);
        comp[find(b)] = find(a);
    }
    for (int64_t n = 0; n < K; ++n) rep.n_components += find(n) == n;
    rep.n_loops = n_edges - K + rep.n_components;
    std::vector<int64_t> parent((size_t)A, -1);
    for (int64_t n = 0; n < K; ++n) {
        if (nodes[n].flags & 4) continue;
        std::sort(adj[n].begin(), adj[n].end());
        for (int64_t a : adj[n])
            if (nodes[a].band < nodes[n].band) { parent[n] = a; break; }
    }
    // open ends: a node with bit 0 goes when every descendant has it too; roots stay
    std::vector<char> keep((size_t)A, 1);
    for (int64_t n = 0; n < K; ++n) keep[n] = !(nodes[n].flags & 1) || parent[n] < 0;
    for (int64_t n = K - 1; n >= 0; --n)
        if (keep[n] && parent[n] >= 0) keep[parent[n]] = 1;
    for (int64_t n = 0; n < K; ++n) rep.n_dropped_open += !keep[n];
    // the points of the tree: the kept nodes, then the terminals behind the kept node their chain reaches
    std::vector<double> xyz((size_t)A * 3), rad((size_t)A);
    for (int64_t n = 0; n < K; ++n) {
        xyz[3 * n] = nodes[n].x; xyz[3 * n + 1] = nodes[n].y; xyz[3 * n + 2] = nodes[n].z;
        rad[n] = nodes[n].radius;
    }
    for (int64_t j = 0; j < T; ++j) {
        int64_t a = terminals[j].node;
        while (!keep[a]) a = parent[a];                                 // a dropped node is no root: it has a parent
        parent[K + j] = a;
        xyz[3 * (K + j)] = terminals[j].x; xyz[3 * (K + j) + 1] = terminals[j].y; xyz[3 * (K + j) + 2] = terminals[j].z;
        rad[K + j] = terminals[j].radius;
    }
    std::vector<int64_t> n_children((size_t)A, 0), root_of((size_t)A, -1);
    std::vector<double> depth((size_t)A, 0.0);
    for (int64_t i = 0; i < A; ++i) {                                   // a parent has a smaller number than its child
        if (!keep[i]) continue;
        if (parent[i] < 0) { root_of[i] = i; ++rep.n_roots; continue; }
        ++n_children[parent[i]];
        root_of[i] = root_of[parent[i]];
        depth[i] = depth[parent[i]] + gap(&xyz[3 * parent[i]], &xyz[3 * i]);
    }

    std::vector<char> state((size_t)A, 0);                              // 1: a point of the output, 2: a pruned leaf
    std::vector<int64_t> at((size_t)A, -1), branch_of((size_t)A, -1), path;
    int64_t n_out = 0, n_branches = 0;
    auto emit = [&](int64_t junction) {                                 // path holds leaf ... first node, back to front
        for (size_t k = path.size(); k-- > 0;) {
            const int64_t i = path[k];
            mm_clpoint& p = out[n_out];
            std::memset(&p, 0, sizeof(p));
            p.x = xyz[3 * i]; p.y = xyz[3 * i + 1]; p.z = xyz[3 * i + 2];
            p.radius = rad[i];
            p.branch_id = (uint32_t)n_branches;
            point_node[n_out] = i;
            at[i] = n_out++;
            branch_of[i] = n_branches;
            state[i] = 1;
        }
        int64_t* info = branch_info + 4 * n_branches;
        info[0] = junction < 0 ? -1 : branch_of[junction];
        info[1] = junction < 0 ? -1 : at[junction];
        info[2] = path.front() >= K;
        info[3] = (int64_t)path.size();
        ++n_branches;
    };
    for (int64_t root = 0; root < K; ++root) {
        if (!keep[root] || parent[root] >= 0) continue;
        std::vector<int64_t> leaves;
        for (int64_t i = root; i < A; ++i)
            if (keep[i] && root_of[i] == root && n_children[i] == 0) leaves.push_back(i);
        int64_t best = leaves[0];                                       // a root without children is its own leaf
        for (int64_t l : leaves)
            if (depth[l] > depth[best]) best = l;
        path.clear();
        for (int64_t i = best; i >= 0; i = parent[i]) path.push_back(i);
        emit(-1);
        for (;;) {
            int64_t pick = -1, pick_junction = -1;
            double pick_len = 0.0;
            for (int64_t l : leaves) {
                if (state[l]) continue;
                path.clear();
                int64_t j = l;
                for (; state[j] != 1; j = parent[j]) path.push_back(j);
                double len = 0.0;                                       // from the junction down, left to right
                int64_t from = j;
                for (size_t k = path.size(); k-- > 0;) {
                    len = len + gap(&xyz[3 * from], &xyz[3 * path[k]]);
                    from = path[k];
                }
                if (pick < 0 || len > pick_len) { pick = l; pick_len = len; pick_junction = j; }
            }
            if (pick < 0) break;
            const double threshold = min_branch_mm >= 0.0 ? min_branch_mm : 2.0 * rad[pick_junction];
            if (pick < K && pick_len < threshold) {
                state[pick] = 2;
                ++rep.n_pruned;
                continue;
            }
            path.clear();
            for (int64_t i = pick; i != pick_junction; i = parent[i]) path.push_back(i);
            emit(pick_junction);
        }
    }
    cl_recompute_tangents(out, n_out);
    rep.n_points = n_out;
    rep.n_branches = n_branches;
    *report = rep;
    return n_out;
}

}  // extern "C"
