// mm_tri_plan.h -- the host plan of the point-to-triangle search (mm_tri_kernels.hip), shared by mm_surface.cpp and
// mm_relax.cpp: the argument checks, the slab order of faces and queries, the faces' kinds, the boxes of query blocks
// and chunks, the (query block, chunk) items with their lower bounds (mm_prune.h) and the staged face records.
// Header-only; internal.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "mm_prune.h"
#include "mm_stage.h"
#include "mm_trace.h"

namespace mm {

// The host side of one call: mm_point_mesh_distance, the host-only test hook mm_tri_plan and step 0 of mm_mesh_relax.
struct TriPlan {
    int qpb = 0, ch = 0;
    std::vector<int32_t> forder;       // staged face j is face forder[j]
    std::vector<int32_t> qperm;        // staged query j is query qperm[j]
    std::vector<uint8_t> degenerate;   // per staged face
    std::vector<uint8_t> thin;         // per staged face: not degenerate and thin (face_kind == 2)
    std::vector<TriWork> work;         // n_a items of pass A (one per query block), then n_b of pass B
    std::vector<Box3> cbox;            // the box of every chunk's corners
    int64_t n_a = 0, n_b = 0;
};

inline int plan_args(const double* vertices, int64_t nv, const int64_t* faces, int64_t nf, const double* queries, int64_t nq,
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

// every component of ab x ac exactly 0, or a repeated index
inline bool is_degenerate(const double* a, const double* b, const double* c, const int64_t* f)
{
    if (f[0] == f[1] || f[1] == f[2] || f[0] == f[2]) return true;
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double nx = ab[1] * ac[2] - ab[2] * ac[1], ny = ab[2] * ac[0] - ab[0] * ac[2], nz = ab[0] * ac[1] - ab[1] * ac[0];
    return nx == 0.0 && ny == 0.0 && nz == 0.0;
}

// The kind of a face as include/mm_ccta.h ("surface distance") states it: 1 degenerate; else 2 (thin) where
// dot(n, n) < 2^-34 (l l) with n = ab x ac and l the largest of dot(ab, ab), dot(ac, ac), dot(bc, bc); else 0.  The values
// are kFaceProper, kFaceDegenerate and kFaceThin of mm_tri_device.h.  Unfused f64 like the degenerate test: the host
// code is built with -ffp-contract=off too.
inline uint8_t face_kind(const double* a, const double* b, const double* c, const int64_t* f)
{
    if (is_degenerate(a, b, c, f)) return 1;
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double bc[3] = {c[0] - b[0], c[1] - b[1], c[2] - b[2]};
    const double nx = ab[1] * ac[2] - ab[2] * ac[1], ny = ab[2] * ac[0] - ab[0] * ac[2], nz = ab[0] * ac[1] - ab[1] * ac[0];
    const double nn = (nx * nx + ny * ny) + nz * nz;
    double l = (ab[0] * ab[0] + ab[1] * ab[1]) + ab[2] * ab[2];
    const double lac = (ac[0] * ac[0] + ac[1] * ac[1]) + ac[2] * ac[2], lbc = (bc[0] * bc[0] + bc[1] * bc[1]) + bc[2] * bc[2];
    l = lac > l ? lac : l;
    l = lbc > l ? lbc : l;
    return nn < 0x1p-34 * (l * l) ? 2 : 0;
}

// Slab order of faces (by centroid: the sum of the three corners) and queries across the longest axis of the faces'
// corners, the boxes of query blocks and chunks, and the items.  Arguments checked by plan_args.
inline int build_plan(const double* v, const int64_t* f, int64_t nf, const double* q, int64_t nq, const char* who, TriPlan& pl)
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
    pl.thin.resize((size_t)nf);
    for (int64_t j = 0; j < nf; ++j) {
        const int64_t* t = f + 3 * (int64_t)pl.forder[(size_t)j];
        const uint8_t kind = face_kind(v + 3 * t[0], v + 3 * t[1], v + 3 * t[2], t);
        pl.degenerate[(size_t)j] = kind == 1;
        pl.thin[(size_t)j] = kind == 2;
    }
    t_order.stop();
    TraceTimer t_items("tri: boxes and items");
    pl.work.clear();
    pl.cbox.clear();
    pl.n_a = pl.n_b = 0;
    if (nq == 0 || nf == 0) return MM_OK;
    const int64_t nqb = (nq + pl.qpb - 1) / pl.qpb, nch = (nf + pl.ch - 1) / pl.ch;
    if (nqb * nch > kMaxIndex) return set_error(MM_ERR_TOO_LARGE, std::string(who) + ": more than 2^31 work items");
    std::vector<Box3> qbox((size_t)nqb);
    std::vector<Box3>& cbox = pl.cbox;
    cbox.assign((size_t)nch, Box3{});
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

// The staged faces: 12 doubles each (a, b, c as x y z w; a.w = the bits of the face's kind, b.w = those of the
// original face index), in the plan's order.
inline void stage_tri_records(const TriPlan& pl, const double* v, const int64_t* f, int64_t nf, double* t)
{
    for (int64_t j = 0; j < nf; ++j, t += 12) {
        const int64_t orig = pl.forder[(size_t)j];
        const unsigned long long w[3] = {pl.degenerate[(size_t)j] ? 1ull : (pl.thin[(size_t)j] ? 2ull : 0ull),
                                         (unsigned long long)orig, 0ull};
        for (int k = 0; k < 3; ++k) {
            std::memcpy(t + 4 * k, v + 3 * f[3 * orig + k], 24);
            std::memcpy(t + 4 * k + 3, &w[k], 8);
        }
    }
}

}  // namespace mm
