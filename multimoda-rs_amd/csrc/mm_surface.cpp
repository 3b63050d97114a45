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
#include "mm_tri_plan.h"

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
    stage_tri_records(pl, vertices_xyz, tris, nf, sp.host<double>(o_tri));
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
