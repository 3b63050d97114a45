// mm_surface.cpp -- surface distance (include/mm_ccta.h, "surface distance"): the squared distance from every query point
// to the nearest triangle of a mesh, with the winning face, the closest point and its region.  The reference bounds this
// quantity inside MeshLab (multimodars/ccta/fixing_functions.py:196-219, checksurfdist / maxsurfdist); here it is a
// measurement of its own.  The host checks the arguments, stages queries and faces in slabs, builds the (query block,
// chunk) work items with their lower bounds, and brings the results back to the caller's order; every distance is
// computed on the device (mm_tri_kernels.hip).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "../../include/mm_ccta.h"
#include "mm_prune.h"
#include "mm_stage.h"
#include "mm_trace.h"

namespace mm {
namespace {

// The host side of one call, shared by mm_point_mesh_distance and the host-only test hook mm_tri_plan.
struct TriPlan {
    int qpb = 0, ch = 0;
    std::vector<int32_t> forder;       // staged face j is face forder[j]
    std::vector<int32_t> qperm;        // staged query j is query qperm[j]
    std::vector<uint8_t> degenerate;   // per staged face
    std::vector<TriWork> work;         // n_a items of pass A (one per query block), then n_b of pass B
    int64_t n_a = 0, n_b = 0;
};

int plan_args(const double* vertices, int64_t nv, const int64_t* faces, int64_t nf, const double* queries, int64_t nq,
              const char* who)
{
    if (nv < 0 || nf < 0 || nq < 0 || (nv > 0 && !vertices) || (nf > 0 && !faces) || (nq > 0 && !queries))
        return set_error(MM_ERR_INVALID, std::string(who) + ": bad arguments");
    if (nv > kMaxIndex || nf > kMaxIndex || nq > kMaxIndex)
        return set_error(MM_ERR_INVALID, std::string(who) + ": nv, nf and nq must stay below 2^31");
    TraceTimer tt("tri: argument checks");
    if (const int rc = faces_in_range(faces, nf, nv, who)) return rc;
    for (int64_t k = 0; k < 3 * nv; ++k)
        if (!std::isfinite(vertices[k])) return set_error(MM_ERR_INVALID, std::string(who) + ": non-finite vertex coordinate");
    for (int64_t k = 0; k < 3 * nq; ++k)
        if (!std::isfinite(queries[k])) return set_error(MM_ERR_INVALID, std::string(who) + ": non-finite query coordinate");
    return MM_OK;
}

// The slack of the bound (mm_prune.h, box_lb2) between a query block q and a chunk's corners c.  The closest point the
// rule computes, u + e t or (a + ab v) + ac w with factors that rounding keeps within a few ulp of [0, 1], lies within a
// few ulp of the largest coordinate of the triangle's own box, hence of the chunk's: each gap is narrowed by 64 such ulp
// (DESIGN 4.19).
double tri_slack(const Box3& q, const Box3& c) { return 64.0 * DBL_EPSILON * std::max(q.largest(), c.largest()); }

// every component of ab x ac exactly 0, or a repeated index
bool is_degenerate(const double* a, const double* b, const double* c, const int64_t* f)
{
    if (f[0] == f[1] || f[1] == f[2] || f[0] == f[2]) return true;
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double nx = ab[1] * ac[2] - ab[2] * ac[1], ny = ab[2] * ac[0] - ab[0] * ac[2], nz = ab[0] * ac[1] - ab[1] * ac[0];
    return nx == 0.0 && ny == 0.0 && nz == 0.0;
}

// Slab order of faces (by centroid: the sum of the three corners) and queries across the longest axis of the faces'
// corners, the boxes of query blocks and chunks, and the items.  Arguments checked by plan_args.
int build_plan(const double* v, const int64_t* f, int64_t nf, const double* q, int64_t nq, const char* who, TriPlan& pl)
{
    pl.qpb = tri_queries_per_block();
    pl.ch = tri_chunk_faces();
    TraceTimer t_order("tri: slab order");
    Box3 all;
    for (int64_t k = 0; k < 3 * nf; ++k) all.add(v + 3 * f[k]);
    const int ax = all.longest_axis();
    std::vector<double> key((size_t)nf);
    for (int64_t i = 0; i < nf; ++i) key[(size_t)i] = (v[3 * f[3 * i] + ax] + v[3 * f[3 * i + 1] + ax]) + v[3 * f[3 * i + 2] + ax];
    slab_permutation(key, pl.forder);
    key.resize((size_t)nq);
    for (int64_t i = 0; i < nq; ++i) key[(size_t)i] = q[3 * i + ax];
    slab_permutation(key, pl.qperm);
    pl.degenerate.resize((size_t)nf);
    for (int64_t j = 0; j < nf; ++j) {
        const int64_t* t = f + 3 * (int64_t)pl.forder[(size_t)j];
        pl.degenerate[(size_t)j] = is_degenerate(v + 3 * t[0], v + 3 * t[1], v + 3 * t[2], t);
    }
    t_order.stop();
    TraceTimer t_items("tri: boxes and items");
    pl.work.clear();
    pl.n_a = pl.n_b = 0;
    if (nq == 0 || nf == 0) return MM_OK;
    const int64_t nqb = (nq + pl.qpb - 1) / pl.qpb, nch = (nf + pl.ch - 1) / pl.ch;
    if (nqb * nch > kMaxIndex) return set_error(MM_ERR_TOO_LARGE, std::string(who) + ": more than 2^31 work items");
    std::vector<Box3> qbox((size_t)nqb), cbox((size_t)nch);
    for (int64_t j = 0; j < nq; ++j) qbox[(size_t)(j / pl.qpb)].add(q + 3 * (int64_t)pl.qperm[(size_t)j]);
    for (int64_t j = 0; j < nf; ++j)
        for (int k = 0; k < 3; ++k) cbox[(size_t)(j / pl.ch)].add(v + 3 * f[3 * (int64_t)pl.forder[(size_t)j] + k]);
    pl.n_a = nqb;
    pl.n_b = nqb * (nch - 1);
    pl.work.resize((size_t)(pl.n_a + pl.n_b));
    std::vector<std::pair<double, int32_t>> cand;
    for (int64_t b = 0; b < nqb; ++b) {
        const Box3& qb = qbox[(size_t)b];
        nearest_first(nch, [&](int64_t c) { return box_lb2(qb, cbox[(size_t)c], tri_slack(qb, cbox[(size_t)c])); }, cand);
        const int32_t q0 = (int32_t)(b * pl.qpb);
        pl.work[(size_t)b] = TriWork{q0, cand[0].second * pl.ch, cand[0].first};
        for (int64_t c = 1; c < nch; ++c)
            pl.work[(size_t)(pl.n_a + b * (nch - 1) + c - 1)] = TriWork{q0, cand[(size_t)c].second * pl.ch, cand[(size_t)c].first};
    }
    return MM_OK;
}

}  // namespace
}  // namespace mm

using namespace mm;

extern "C" {

int mm_tri_plan(const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf, const double* queries_xyz,
                int64_t nq, int32_t* face_order, int32_t* query_perm, int64_t* info, int32_t* items, double* item_lb2,
                int64_t cap)
{
    if (!info || cap < 0 || (cap > 0 && (!items || !item_lb2)) || (nf > 0 && !face_order) || (nq > 0 && !query_perm))
        return set_error(MM_ERR_INVALID, "mm_tri_plan: bad arguments");
    int rc = plan_args(vertices_xyz, nv, tris, nf, queries_xyz, nq, "mm_tri_plan");
    if (rc) return rc;
    TriPlan pl;
    if ((rc = build_plan(vertices_xyz, tris, nf, queries_xyz, nq, "mm_tri_plan", pl))) return rc;
    if (nf > 0) std::memcpy(face_order, pl.forder.data(), (size_t)nf * 4);
    if (nq > 0) std::memcpy(query_perm, pl.qperm.data(), (size_t)nq * 4);
    info[0] = pl.n_a; info[1] = pl.n_b; info[2] = pl.qpb; info[3] = pl.ch;
    for (int64_t k = 0; k < std::min<int64_t>(cap, pl.n_a + pl.n_b); ++k) {
        const TriWork& w = pl.work[(size_t)k];
        items[3 * k] = k < pl.n_a ? 0 : 1; items[3 * k + 1] = w.q0; items[3 * k + 2] = w.c0;
        item_lb2[k] = w.lb2;
    }
    return MM_OK;
}

int mm_point_mesh_distance(mm_engine* h, const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf,
                           const double* queries_xyz, int64_t nq, double* out_sq, int64_t* out_face, double* out_closest,
                           int32_t* out_region, mm_surface_report* report)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (!report || (nq > 0 && !out_sq)) return set_error(MM_ERR_INVALID, "mm_point_mesh_distance: bad arguments");
    if ((rc = plan_args(vertices_xyz, nv, tris, nf, queries_xyz, nq, "mm_point_mesh_distance"))) return rc;
    std::memset(report, 0, sizeof(*report));
    if (nq == 0) return MM_OK;
    if (nf == 0) {                                                     // no face beat anything
        for (int64_t i = 0; i < nq; ++i) {
            out_sq[i] = INFINITY;
            if (out_face) out_face[i] = -1;
            if (out_closest) out_closest[3 * i] = out_closest[3 * i + 1] = out_closest[3 * i + 2] = NAN;
            if (out_region) out_region[i] = -1;
        }
        return MM_OK;
    }
    TriPlan pl;
    if ((rc = build_plan(vertices_xyz, tris, nf, queries_xyz, nq, "mm_point_mesh_distance", pl))) return rc;

    StagedPass sp;
    const size_t o_tri = sp.in.take((size_t)nf * 96), o_q = sp.in.take((size_t)nq * 24);
    const size_t o_work = sp.in.take(pl.work.size() * sizeof(TriWork));
    const size_t o_sq = sp.out.take((size_t)nq * 8), o_key = sp.out.take((size_t)nq * 8), o_cl = sp.out.take((size_t)nq * 24);
    const size_t o_reg = sp.out.take((size_t)nq * 4), o_cnt = sp.out.take(8);
    if ((rc = sp.reserve(e))) return rc;
    double* t = sp.host<double>(o_tri);
    for (int64_t j = 0; j < nf; ++j, t += 12) {
        const int64_t orig = pl.forder[(size_t)j];
        const unsigned long long w[3] = {pl.degenerate[(size_t)j] ? 1ull : 0ull, (unsigned long long)orig, 0ull};
        for (int k = 0; k < 3; ++k) {
            std::memcpy(t + 4 * k, vertices_xyz + 3 * tris[3 * orig + k], 24);
            std::memcpy(t + 4 * k + 3, &w[k], 8);
        }
    }
    double* sq = sp.host<double>(o_q);
    for (int64_t j = 0; j < nq; ++j) std::memcpy(sq + 3 * j, queries_xyz + 3 * (int64_t)pl.qperm[(size_t)j], 24);
    std::memcpy(sp.host<TriWork>(o_work), pl.work.data(), pl.work.size() * sizeof(TriWork));
    rc = sp.run((double)nq * (double)nf, "launch_tri_distance", [&] {
        return launch_tri_distance(sp.dev_in<TriWork>(o_work), (int)pl.n_a, (int)pl.n_b, sp.dev_in<double>(o_tri), (int)nf,
                                   sp.dev_in<double>(o_q), (int)nq, sp.dev_out<unsigned long long>(o_sq),
                                   sp.dev_out<unsigned long long>(o_key), sp.dev_out<double>(o_cl),
                                   sp.dev_out<int32_t>(o_reg), sp.dev_out<unsigned long long>(o_cnt), e->stream);
    });
    if (rc) return rc;
    const double* d_sq = sp.host<double>(o_sq);
    const unsigned long long* d_key = sp.host<unsigned long long>(o_key);
    const double* d_cl = sp.host<double>(o_cl);
    const int32_t* d_reg = sp.host<int32_t>(o_reg);
    for (int64_t j = 0; j < nq; ++j) {
        const int64_t i = pl.qperm[(size_t)j];
        out_sq[i] = d_sq[j];
        if (out_face) out_face[i] = d_key[j] == ~0ull ? -1 : (int64_t)(d_key[j] >> 32);
        if (out_closest) std::memcpy(out_closest + 3 * i, d_cl + 3 * j, 24);
        if (out_region) out_region[i] = d_reg[j];
    }
    report->items_pass_a = pl.n_a;
    report->items_pass_b = pl.n_b;
    report->items_skipped = (int64_t)*sp.host<unsigned long long>(o_cnt);
    report->n_launches = tri_launches((int)pl.n_b);
    report->bytes_uploaded = (int64_t)sp.in.size();
    report->bytes_downloaded = (int64_t)sp.out.size();
    return MM_OK;
}

}  // extern "C"
