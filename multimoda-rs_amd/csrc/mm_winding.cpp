// mm_winding.cpp -- winding numbers (include/mm_ccta.h, "winding number"): the generalized winding number of a triangle
// mesh at query points, as quarter turns and a complex remainder per query.  The host checks the arguments, removes the
// degenerate faces, stages the others in the caller's order, and turns the device's (n, p, rho, touch) into w and err;
// every face is folded on the device (mm_winding_kernels.hip).  mm_winding_fold_host runs the same arithmetic
// (mm_winding_device.h) on the CPU for the tests.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mm_ccta.h"
#include "mm_tri_plan.h"
#include "mm_winding_device.h"

using namespace mm;

namespace {

constexpr double kMaxCoord = 0x1p300;

struct WindPlan {
    int64_t chunk = 0, per_group = 0, groups = 0, staged = 0;
};

// the grouping of the rule: G = ceil(chunks / 16) consecutive chunks a group
WindPlan wind_plan(int64_t staged)
{
    WindPlan pl;
    pl.chunk = winding::kChunk;
    pl.staged = staged;
    const int64_t chunks = (staged + pl.chunk - 1) / pl.chunk;
    pl.per_group = (chunks + winding::kMaxGroups - 1) / winding::kMaxGroups;
    pl.groups = pl.per_group ? (chunks + pl.per_group - 1) / pl.per_group : 0;
    return pl;
}

int wind_args(const double* v, int64_t nv, const int64_t* f, int64_t nf, const double* q, int64_t nq, const char* who)
{
    if (const int rc = plan_args(v, nv, f, nf, q, nq, who)) return rc;
    for (int64_t k = 0; k < 3 * nv; ++k)
        if (std::fabs(v[k]) > kMaxCoord) return set_error(MM_ERR_INVALID, std::string(who) + ": vertex coordinate above 2^300");
    for (int64_t k = 0; k < 3 * nq; ++k)
        if (std::fabs(q[k]) > kMaxCoord) return set_error(MM_ERR_INVALID, std::string(who) + ": query coordinate above 2^300");
    return MM_OK;
}

// the faces that are not degenerate, in the caller's order
void staged_faces(const double* v, const int64_t* f, int64_t nf, std::vector<int64_t>& keep)
{
    keep.clear();
    for (int64_t i = 0; i < nf; ++i) {
        const int64_t* t = f + 3 * i;
        if (!is_degenerate(v + 3 * t[0], v + 3 * t[1], v + 3 * t[2], t)) keep.push_back(i);
    }
}

void stage_tri9(const double* v, const int64_t* f, const std::vector<int64_t>& keep, double* t)
{
    for (const int64_t i : keep)
        for (int k = 0; k < 3; ++k, t += 3) std::memcpy(t, v + 3 * f[3 * i + k], 24);
}

void no_face(int64_t nq, int32_t* out_n, double* out_p, double* out_rho, uint8_t* out_touch)
{
    for (int64_t i = 0; i < nq; ++i) {
        out_n[i] = 0; out_p[2 * i] = 1.0; out_p[2 * i + 1] = 0.0; out_rho[i] = INFINITY; out_touch[i] = 0;
    }
}

}  // namespace

extern "C" {

int mm_winding_plan(int64_t n_staged, int64_t* info)
{
    if (!info || n_staged < 0 || n_staged > kMaxIndex) return set_error(MM_ERR_INVALID, "mm_winding_plan: bad arguments");
    const WindPlan pl = wind_plan(n_staged);
    info[0] = pl.chunk; info[1] = pl.per_group; info[2] = pl.groups; info[3] = pl.staged;
    return MM_OK;
}

int mm_winding_fold_host(const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf, const double* queries_xyz,
                         int64_t nq, int32_t* out_n, double* out_p, double* out_rho, uint8_t* out_touch, int64_t* n_staged)
{
    if (!n_staged || (nq > 0 && (!out_n || !out_p || !out_rho || !out_touch)))
        return set_error(MM_ERR_INVALID, "mm_winding_fold_host: bad arguments");
    if (const int rc = wind_args(vertices_xyz, nv, tris, nf, queries_xyz, nq, "mm_winding_fold_host")) return rc;
    std::vector<int64_t> keep;
    staged_faces(vertices_xyz, tris, nf, keep);
    const WindPlan pl = wind_plan((int64_t)keep.size());
    *n_staged = pl.staged;
    if (pl.staged == 0) { no_face(nq, out_n, out_p, out_rho, out_touch); return MM_OK; }
    std::vector<double> t9((size_t)pl.staged * 9);
    stage_tri9(vertices_xyz, tris, keep, t9.data());
    const int64_t per = pl.per_group * pl.chunk;
    for (int64_t i = 0; i < nq; ++i) {
        const double* p = queries_xyz + 3 * i;
        winding::State total = winding::start();
        for (int64_t g = 0; g < pl.groups; ++g) {
            winding::State s = winding::start();
            for (int64_t j = g * per; j < std::min(pl.staged, (g + 1) * per); ++j) {
                const double* t = t9.data() + 9 * j;
                winding::face(s, p[0], p[1], p[2], t[0], t[1], t[2], t[3], t[4], t[5], t[6], t[7], t[8]);
            }
            if (g == 0) total = s;
            else winding::join(total, s);
        }
        out_n[i] = total.n; out_p[2 * i] = total.pr; out_p[2 * i + 1] = total.pi; out_rho[i] = total.rho;
        out_touch[i] = (uint8_t)total.touch;
    }
    return MM_OK;
}

int mm_winding_result(const int32_t* n, const double* p, const double* rho, const uint8_t* touch, int64_t nq, int64_t n_staged,
                      double* out_w, double* out_err)
{
    if (nq < 0 || n_staged < 0 || (nq > 0 && (!n || !p || !rho || !touch || !out_w || !out_err)))
        return set_error(MM_ERR_INVALID, "mm_winding_result: bad arguments");
    for (int64_t i = 0; i < nq; ++i) {
        out_w[i] = ((double)n[i] * M_PI_2 + std::atan2(p[2 * i + 1], p[2 * i])) / (2.0 * M_PI);
        const bool proven = !touch[i] && rho[i] >= MM_WINDING_RHO_MIN;
        out_err[i] = proven ? (double)n_staged * (MM_WINDING_ERR_C1 + MM_WINDING_ERR_C2 / rho[i]) * 0x1p-53 : INFINITY;
    }
    return MM_OK;
}

int mm_mesh_winding(mm_engine* h, const double* vertices_xyz, int64_t nv, const int64_t* tris, int64_t nf,
                    const double* queries_xyz, int64_t nq, int32_t* out_n, double* out_p, double* out_rho, uint8_t* out_touch,
                    mm_winding_report* report)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (!report || (nq > 0 && (!out_n || !out_p || !out_rho || !out_touch)))
        return set_error(MM_ERR_INVALID, "mm_mesh_winding: bad arguments");
    if ((rc = wind_args(vertices_xyz, nv, tris, nf, queries_xyz, nq, "mm_mesh_winding"))) return rc;
    std::memset(report, 0, sizeof(*report));
    std::vector<int64_t> keep;
    staged_faces(vertices_xyz, tris, nf, keep);
    const WindPlan pl = wind_plan((int64_t)keep.size());
    report->n_staged_faces = pl.staged;
    report->n_degenerate_faces = nf - pl.staged;
    report->chunk_faces = pl.chunk;
    report->chunks_per_group = pl.per_group;
    report->groups = pl.groups;
    if (nq == 0) return MM_OK;
    if (pl.staged == 0) { no_face(nq, out_n, out_p, out_rho, out_touch); return MM_OK; }
    const int64_t qblocks = (nq + wind_queries_per_block() - 1) / wind_queries_per_block();
    if (qblocks * pl.groups > kMaxIndex) return set_error(MM_ERR_TOO_LARGE, "mm_mesh_winding: more than 2^31 work items");

    StagedPass sp;
    const size_t o_tri = sp.in.take((size_t)pl.staged * 72), o_q = sp.in.take((size_t)nq * 24);
    const size_t o_n = sp.out.take((size_t)nq * 4), o_p = sp.out.take((size_t)nq * 16), o_rho = sp.out.take((size_t)nq * 8);
    const size_t o_touch = sp.out.take((size_t)nq * 4);
    const size_t o_part = sp.scratch.take((size_t)nq * (size_t)pl.groups * sizeof(winding::State));
    if ((rc = sp.reserve(e))) return rc;
    stage_tri9(vertices_xyz, tris, keep, sp.host<double>(o_tri));
    std::memcpy(sp.host<double>(o_q), queries_xyz, (size_t)nq * 24);
    rc = sp.run((double)nq * (double)pl.staged, "launch_winding", [&] {
        return launch_winding(sp.dev_in<double>(o_tri), (int)pl.staged, (int)pl.per_group, (int)pl.groups, sp.dev_in<double>(o_q),
                              (int)nq, sp.dev_scratch<void>(o_part), sp.dev_out<int32_t>(o_n), sp.dev_out<double>(o_p),
                              sp.dev_out<double>(o_rho), sp.dev_out<int32_t>(o_touch), e->stream);
    });
    if (rc) return rc;
    std::memcpy(out_n, sp.host<int32_t>(o_n), (size_t)nq * 4);
    std::memcpy(out_p, sp.host<double>(o_p), (size_t)nq * 16);
    std::memcpy(out_rho, sp.host<double>(o_rho), (size_t)nq * 8);
    const int32_t* touch = sp.host<int32_t>(o_touch);
    for (int64_t i = 0; i < nq; ++i) out_touch[i] = touch[i] != 0;
    report->items = qblocks * pl.groups;
    report->n_launches = wind_launches();
    report->bytes_uploaded = (int64_t)sp.in.size();
    report->bytes_downloaded = (int64_t)sp.out.size();
    report->bytes_scratch = (int64_t)sp.scratch.size();
    return MM_OK;
}

}  // extern "C"
