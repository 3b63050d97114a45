// mm_intersect.cpp -- mesh intersections (include/mm_ccta.h, "mesh intersections"): which pairs of faces of one mesh, or
// of two, are not proved disjoint.  The reference leaves the question to MeshLab and switches it off
// (multimodars/ccta/fixing_functions.py:182-185, 234); here it is a report of its own.  The host checks the arguments,
// gives every vertex its canonical id, stages the faces in slabs (mm_prune.h), keeps the chunk pairs whose boxes overlap
// and sorts the pairs that come back; every pair of faces is tested on the device (mm_intersect_kernels.hip).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/mm_ccta.h"
#include "mm_tri_plan.h"

using namespace mm;

namespace {

struct IsectMesh {
    const double* v = nullptr;
    const int64_t* f = nullptr;
    int64_t nv = 0, nf = 0;
    std::vector<int32_t> order;        // staged face j is face order[j]
    std::vector<int32_t> canon;        // per vertex its canonical id (self form; empty: the index itself)
    std::vector<uint8_t> degenerate;   // per staged face
    std::vector<Box3> cbox;            // the box of every chunk's corners, as TriPlan::cbox
    int64_t id(int64_t vertex) const { return canon.empty() ? vertex : canon[(size_t)vertex]; }
    int64_t chunk_faces(int64_t c, int ch) const { return std::min<int64_t>(ch, nf - c * ch); }
};

struct IsectPlan {
    int ch = 0;
    bool self_form = true;
    IsectMesh a, b;                    // self form: b stays empty
    std::vector<int32_t> items;        // (I, J) chunk pairs with overlapping boxes
    int64_t items_total = 0, pair_box_tests = 0, n_degenerate = 0;
    const IsectMesh& second() const { return self_form ? a : b; }
};

// the lowest index with equal coordinates, +0.0 == -0.0
void canonical_ids(const double* v, int64_t nv, std::vector<int32_t>& canon)
{
    std::vector<int32_t> idx((size_t)nv);
    for (int64_t i = 0; i < nv; ++i) idx[(size_t)i] = (int32_t)i;
    auto less = [v](int32_t i, int32_t j) {
        for (int k = 0; k < 3; ++k) {
            const double x = v[3 * (int64_t)i + k], y = v[3 * (int64_t)j + k];   // -0.0 < +0.0 is false both ways
            if (x < y) return true;
            if (y < x) return false;
        }
        return i < j;
    };
    std::sort(idx.begin(), idx.end(), less);
    canon.resize((size_t)nv);
    int32_t first = 0;
    for (int64_t k = 0; k < nv; ++k) {
        const int32_t i = idx[(size_t)k];
        const double *x = v + 3 * (int64_t)first, *y = v + 3 * (int64_t)i;
        if (k == 0 || x[0] != y[0] || x[1] != y[1] || x[2] != y[2]) first = i;   // a run starts at its lowest index
        canon[(size_t)i] = first;
    }
}

void order_mesh(IsectMesh& m, int ax, int ch)
{
    const double* v = m.v;
    const int64_t* f = m.f;
    std::vector<double> key((size_t)m.nf);
    for (int64_t i = 0; i < m.nf; ++i) key[(size_t)i] = (v[3 * f[3 * i] + ax] + v[3 * f[3 * i + 1] + ax]) + v[3 * f[3 * i + 2] + ax];
    slab_permutation(key, m.order);
    m.degenerate.resize((size_t)m.nf);
    m.cbox.assign((size_t)((m.nf + ch - 1) / ch), Box3{});
    for (int64_t j = 0; j < m.nf; ++j) {
        const int64_t* t = f + 3 * (int64_t)m.order[(size_t)j];
        const int64_t ids[3] = {m.id(t[0]), m.id(t[1]), m.id(t[2])};
        m.degenerate[(size_t)j] = is_degenerate(v + 3 * t[0], v + 3 * t[1], v + 3 * t[2], ids);
        for (int k = 0; k < 3; ++k) m.cbox[(size_t)(j / ch)].add(v + 3 * t[k]);
    }
}

bool boxes_overlap(const Box3& x, const Box3& y)
{
    for (int k = 0; k < 3; ++k)
        if (x.lo[k] > y.hi[k] || y.lo[k] > x.hi[k]) return false;
    return true;
}

int check_meshes(const double* va, int64_t nva, const int64_t* fa, int64_t nfa, const double* vb, int64_t nvb,
                 const int64_t* fb, int64_t nfb, const char* who)
{
    int rc = plan_args(va, nva, fa, nfa, nullptr, 0, who);
    if (rc) return rc;
    if (!vb) return MM_OK;
    return plan_args(vb, nvb, fb, nfb, nullptr, 0, who);
}

// Arguments checked by check_meshes.  vb == NULL: the self form.
int build_isect_plan(const double* va, int64_t nva, const int64_t* fa, int64_t nfa, const double* vb, int64_t nvb,
                     const int64_t* fb, int64_t nfb, const char* who, IsectPlan& pl)
{
    pl.ch = isect_chunk_faces();
    pl.self_form = vb == nullptr;
    pl.a.v = va; pl.a.f = fa; pl.a.nv = nva; pl.a.nf = nfa;
    if (!pl.self_form) { pl.b.v = vb; pl.b.f = fb; pl.b.nv = nvb; pl.b.nf = nfb; }
    TraceTimer t_order("isect: ids and slab order");
    if (pl.self_form) canonical_ids(va, nva, pl.a.canon);
    Box3 all;
    for (int64_t k = 0; k < 3 * nfa; ++k) all.add(va + 3 * fa[k]);
    for (int64_t k = 0; k < 3 * pl.b.nf; ++k) all.add(vb + 3 * fb[k]);
    const int ax = all.longest_axis();
    order_mesh(pl.a, ax, pl.ch);
    if (!pl.self_form) order_mesh(pl.b, ax, pl.ch);
    pl.n_degenerate = 0;
    for (uint8_t d : pl.a.degenerate) pl.n_degenerate += d;
    for (uint8_t d : pl.b.degenerate) pl.n_degenerate += d;
    t_order.stop();
    TraceTimer t_items("isect: items");
    const IsectMesh& s = pl.second();
    const int64_t nca = (int64_t)pl.a.cbox.size(), ncb = (int64_t)s.cbox.size();
    pl.items.clear();
    pl.items_total = pl.self_form ? nca * (nca + 1) / 2 : nca * ncb;
    pl.pair_box_tests = 0;
    for (int64_t i = 0; i < nca; ++i)
        for (int64_t j = pl.self_form ? i : 0; j < ncb; ++j) {
            if (!boxes_overlap(pl.a.cbox[(size_t)i], s.cbox[(size_t)j])) continue;
            if ((int64_t)pl.items.size() / 2 >= kMaxIndex)
                return set_error(MM_ERR_TOO_LARGE, std::string(who) + ": more than 2^31 - 1 work items");
            pl.items.push_back((int32_t)i);
            pl.items.push_back((int32_t)j);
            const int64_t ni = pl.a.chunk_faces(i, pl.ch), nj = s.chunk_faces(j, pl.ch);
            pl.pair_box_tests += pl.self_form && i == j ? ni * (ni - 1) / 2 : ni * nj;
        }
    return MM_OK;
}

// 12 doubles a face: a, b, c as x y z w; a.w = id(a) | id(b) << 32, b.w = id(c) | original index << 32, c.w = degenerate
void stage_isect_records(const IsectMesh& m, double* t)
{
    for (int64_t j = 0; j < m.nf; ++j, t += 12) {
        const int64_t orig = m.order[(size_t)j];
        const int64_t* f = m.f + 3 * orig;
        const unsigned long long w[3] = {(unsigned long long)(uint32_t)m.id(f[0]) | (unsigned long long)(uint32_t)m.id(f[1]) << 32,
                                         (unsigned long long)(uint32_t)m.id(f[2]) | (unsigned long long)orig << 32,
                                         m.degenerate[(size_t)j] ? 1ull : 0ull};
        for (int k = 0; k < 3; ++k) {
            std::memcpy(t + 4 * k, m.v + 3 * f[k], 24);
            std::memcpy(t + 4 * k + 3, &w[k], 8);
        }
    }
}

}  // namespace

extern "C" {

int mm_isect_plan(const double* va, int64_t nva, const int64_t* fa, int64_t nfa, const double* vb, int64_t nvb,
                  const int64_t* fb, int64_t nfb, int32_t* order_a, int32_t* order_b, int64_t* info, double* chunk_boxes,
                  int32_t* items, int64_t cap)
{
    if (!info || cap < 0 || (cap > 0 && !items) || (nfa > 0 && !order_a) || (vb && nfb > 0 && !order_b))
        return set_error(MM_ERR_INVALID, "mm_isect_plan: bad arguments");
    int rc = check_meshes(va, nva, fa, nfa, vb, nvb, fb, nfb, "mm_isect_plan");
    if (rc) return rc;
    IsectPlan pl;
    if ((rc = build_isect_plan(va, nva, fa, nfa, vb, nvb, fb, nfb, "mm_isect_plan", pl))) return rc;
    if (nfa > 0) std::memcpy(order_a, pl.a.order.data(), (size_t)nfa * 4);
    if (pl.b.nf > 0) std::memcpy(order_b, pl.b.order.data(), (size_t)pl.b.nf * 4);
    const int64_t n = (int64_t)pl.items.size() / 2;
    info[0] = n; info[1] = pl.items_total; info[2] = pl.ch;
    info[3] = (int64_t)pl.a.cbox.size(); info[4] = (int64_t)pl.b.cbox.size();
    if (chunk_boxes) {
        if (!pl.a.cbox.empty()) std::memcpy(chunk_boxes, pl.a.cbox.data(), pl.a.cbox.size() * sizeof(Box3));
        if (!pl.b.cbox.empty()) std::memcpy(chunk_boxes + 6 * pl.a.cbox.size(), pl.b.cbox.data(), pl.b.cbox.size() * sizeof(Box3));
    }
    if (std::min(cap, n) > 0) std::memcpy(items, pl.items.data(), (size_t)std::min(cap, n) * 8);
    return MM_OK;
}

int mm_mesh_intersections(mm_engine* h, const double* va, int64_t nva, const int64_t* fa, int64_t nfa, const double* vb,
                          int64_t nvb, const int64_t* fb, int64_t nfb, int64_t max_pairs, uint8_t* out_state_a,
                          uint8_t* out_state_b, int64_t* out_pairs, int8_t* out_pair_state, mm_intersect_report* report)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    const bool self_form = vb == nullptr;
    if (!report || max_pairs < 0 || (nfa > 0 && !out_state_a) || (!self_form && nfb > 0 && !out_state_b))
        return set_error(MM_ERR_INVALID, "mm_mesh_intersections: bad arguments");
    if ((rc = check_meshes(va, nva, fa, nfa, vb, nvb, fb, nfb, "mm_mesh_intersections"))) return rc;
    IsectPlan pl;
    if ((rc = build_isect_plan(va, nva, fa, nfa, vb, nvb, fb, nfb, "mm_mesh_intersections", pl))) return rc;
    const int64_t nb = pl.b.nf, n_items = (int64_t)pl.items.size() / 2;
    const int64_t cap = out_pairs && out_pair_state ? max_pairs : 0;

    std::memset(report, 0, sizeof(*report));
    if (nfa > 0) std::memset(out_state_a, 0, (size_t)nfa);
    if (nb > 0) std::memset(out_state_b, 0, (size_t)nb);
    report->n_degenerate_faces = pl.n_degenerate;
    report->items = n_items;
    report->items_total = pl.items_total;
    report->pair_box_tests = pl.pair_box_tests;
    report->pairs_complete = 1;
    if (n_items == 0) return MM_OK;

    const int64_t dev_cap = std::min(cap, pl.pair_box_tests);       // no call finds more pairs than it tests
    StagedPass sp;
    const size_t n_rec = (size_t)(nfa + nb);
    const size_t o_tri = sp.in.take(n_rec * 96), o_items = sp.in.take((size_t)n_items * 8);
    const size_t o_state = sp.out.take(n_rec), o_cnt = sp.out.take(64), o_pairs = sp.out.take((size_t)dev_cap * 8);
    if ((rc = sp.reserve(e))) return rc;
    stage_isect_records(pl.a, sp.host<double>(o_tri));
    if (nb > 0) stage_isect_records(pl.b, sp.host<double>(o_tri) + 12 * nfa);
    std::memcpy(sp.host<int32_t>(o_items), pl.items.data(), (size_t)n_items * 8);
    MM_TRY_HIP(hipMemcpyAsync(sp.d, sp.h, sp.in.size(), hipMemcpyHostToDevice, e->stream));
    if ((rc = e->profile_begin(e->stream))) return rc;
    const hipError_t he = launch_isect_pairs(sp.dev_in<int32_t>(o_items), (int)n_items, sp.dev_in<double>(o_tri), (int)nfa,
                                             (int)(self_form ? nfa : nb), self_form ? 0 : (int)nfa, self_form,
                                             sp.dev_out<unsigned int>(o_state), (long long)(up256(n_rec) / 4),
                                             sp.dev_out<unsigned long long>(o_cnt), sp.dev_out<unsigned long long>(o_pairs),
                                             (unsigned long long)dev_cap, e->stream);
    if (he != hipSuccess) return hip_error(he, "launch_isect_pairs");
    if ((rc = e->profile_end(e->stream, (double)pl.pair_box_tests, 0))) return rc;
    MM_TRY_HIP(hipMemcpyAsync(sp.h, sp.dev_out<unsigned char>(0), o_cnt + 64, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    const unsigned long long* cnt = sp.host<unsigned long long>(o_cnt);
    const int64_t n_pairs = (int64_t)cnt[4];
    if (cnt[0] + cnt[1] != cnt[4] || n_pairs < 0 || n_pairs > pl.pair_box_tests)
        return set_error(MM_ERR_HIP, "mm_mesh_intersections: pair counters out of range");
    const bool complete = n_pairs <= cap;
    if (complete && n_pairs > 0) {
        MM_TRY_HIP(hipMemcpyAsync(sp.host<unsigned char>(o_pairs), sp.dev_out<unsigned char>(o_pairs), (size_t)n_pairs * 8,
                                  hipMemcpyDeviceToHost, e->stream));
        MM_TRY_HIP(hipStreamSynchronize(e->stream));
    }
    const uint8_t* st = sp.host<uint8_t>(o_state);
    for (int64_t j = 0; j < nfa; ++j) out_state_a[pl.a.order[(size_t)j]] = st[j];
    for (int64_t j = 0; j < nb; ++j) out_state_b[pl.b.order[(size_t)j]] = st[nfa + j];
    report->n_intersecting_pairs = (int64_t)cnt[0];
    report->n_undecided_pairs = (int64_t)cnt[1];
    report->n_coincident_pairs = (int64_t)cnt[2];
    report->narrow_tests = (int64_t)cnt[3];
    report->n_launches = isect_launches();
    report->bytes_uploaded = (int64_t)sp.in.size();
    report->bytes_downloaded = (int64_t)(o_cnt + 256) + (complete ? n_pairs * 8 : 0);
    report->pairs_complete = complete ? 1 : 0;
    if (complete && n_pairs > 0) {
        unsigned long long* rec = sp.host<unsigned long long>(o_pairs);
        constexpr unsigned long long mask = (1ull << 62) - 1;
        std::sort(rec, rec + n_pairs, [](unsigned long long x, unsigned long long y) { return (x & mask) < (y & mask); });
        for (int64_t k = 0; k < n_pairs; ++k) {
            out_pairs[2 * k] = (int64_t)((rec[k] & mask) >> 31);
            out_pairs[2 * k + 1] = (int64_t)(rec[k] & 0x7fffffffull);
            out_pair_state[k] = (int8_t)(rec[k] >> 62);
        }
    }
    return MM_OK;
}

}  // extern "C"
