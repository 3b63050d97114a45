// mm_ccta.cpp -- CCTA diameter search (include/mm_ccta.h): 41 radial scalings x symmetric RMS
// nearest-neighbour distance in 3-D.  Every nearest-neighbour minimum is computed on the device in
// exact f64 (mm_nn_kernels.hip, one batch per search); morphing, sums and selection are host f64
// in the reference's operation order (-ffp-contract=off).  Reference:
// src/ccta/adjust_mesh/scale_coronary.rs (lines cited per function).
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <numeric>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/mm_ccta.h"
#include "mm_adjacency.h"
#include "mm_prune.h"
#include "mm_stage.h"
#include "mm_pool.h"
#include "mm_trace.h"

namespace mm {
namespace {

// AoS triples.  A derived set (unit != nullptr) is xyz moved by adj along per-point unit vectors where has[i]
// (centerline_based_diameter_morphing, scale_coronary.rs:236-239): it is never materialised on the host --
// the device computes it from the base points and the unit vectors staged once for all scalings.
struct Set3 {
    const double* xyz; int64_t n;
    const double* unit = nullptr; const uint8_t* has = nullptr; double adj = 0.0;
    double at(int64_t i, int a) const {
        return (unit && has[i]) ? xyz[3 * i + a] + unit[3 * i + a] * adj : xyz[3 * i + a];   // :236 p + unit * x
    }
};

// Slab order of a point set (mm_prune.h, slab_permutation) along the longest axis of its bounding box.  The sets here are
// vessel surfaces -- thin shells around a centerline -- and their nearest neighbours are radial, i.e. in the same or the
// next slab; boxes of compact 3-D patches (k-d leaves, Morton runs) overlap their neighbours and the opposite wall and
// prune far less (measured on the bench case: pass B 6.1 ms with Morton runs, 3.5 ms with k-d leaves, 2.5 ms with slabs).
void slab_order(const Set3& st, std::vector<int32_t>& perm)
{
    Box3 all;
    for (int64_t i = 0; i < st.n; ++i) { const double v[3] = {st.at(i, 0), st.at(i, 1), st.at(i, 2)}; all.add(v); }
    const int ax = all.longest_axis();
    std::vector<double> key((size_t)st.n);
    for (int64_t i = 0; i < st.n; ++i) key[(size_t)i] = st.at(i, ax);
    slab_permutation(key, perm);
}

// The host side of a nearest-neighbour batch, shared by the launch paths (nn_batch_view, radius_counts) and the
// host-only test hook mm_nn_plan: the staging order of every set, the point-pool layout, the device pairs, the bounding
// box of every group of qpb staged points, and the (query block, chunk) work items of each pair.
constexpr int64_t kSortMin = 4096;   // smaller sets: original order, every chunk scanned

struct NnPlan {
    int qpb = 0, ch = 0, span = 0;
    std::vector<int64_t> soff;                 // point-pool offset of every set
    std::vector<int32_t> perm_of;              // set -> its entry of perms (-1: staged in original order)
    std::vector<std::vector<int32_t>> perms;   // slab orders, one per distinct base set
    std::vector<int64_t> perm_off;             // offset of every entry of perms in the permutation pool
    std::vector<NnPair> hp;                   // device pairs: both sets non-empty
    std::vector<int> owner;                    // device pair -> caller's pair
    int64_t nout = 0;
    std::vector<int64_t> goff;                 // first group of every set
    std::vector<Box3> box;                     // of every group (filled by nn_plan_stage_set)
    int64_t npts() const { return soff.back(); }
};

// Validates the pairs, sorts the large sets and lays out the pools.  order_like (nullable, one entry per set): the
// set whose spatial order this one shares -- a morphed copy of a set moves every point by at most a few mm, so the 41
// scalings of a search reuse one sort.
int nn_plan_pairs(const std::vector<Set3>& sets, const std::vector<std::array<int32_t, 2>>& pr,
                  const std::vector<int32_t>* order_like, const char* what, NnPlan& pl)
{
    const size_t S = sets.size();
    for (size_t k = 0; k < pr.size(); ++k)
        if (pr[k][0] < 0 || pr[k][1] < 0 || (size_t)pr[k][0] >= S || (size_t)pr[k][1] >= S)
            return set_error(MM_ERR_INVALID, std::string(what) + ": set index out of range");
    pl.qpb = nn_queries_per_block(); pl.ch = nn_chunk_points(); pl.span = nn_span_chunks();
    pl.soff.assign(S + 1, 0);
    for (size_t s = 0; s < S; ++s) pl.soff[s + 1] = pl.soff[s] + sets[s].n;

    // ---- spatial orders: one sort per distinct base set ---------------------------------------
    std::vector<int32_t> base(S, -1);
    std::vector<int32_t> bases;   // distinct sets that get sorted
    for (size_t s = 0; s < S; ++s) {
        if (sets[s].n < kSortMin) continue;
        int32_t b = order_like ? (*order_like)[s] : (int32_t)s;
        if (b < 0 || (size_t)b >= S || sets[(size_t)b].n != sets[s].n) b = (int32_t)s;
        base[s] = b;
        if (std::find(bases.begin(), bases.end(), b) == bases.end()) bases.push_back(b);
    }
    pl.perms.assign(bases.size(), {});
    { TraceTimer tt("nn: slab order");
    parallel_for((int)bases.size(), [&](int k) { slab_order(sets[(size_t)bases[(size_t)k]], pl.perms[(size_t)k]); });
    }
    pl.perm_off.assign(bases.size() + 1, 0);
    for (size_t k = 0; k < bases.size(); ++k) pl.perm_off[k + 1] = pl.perm_off[k] + (int64_t)pl.perms[k].size();
    pl.perm_of.assign(S, -1);
    for (size_t s = 0; s < S; ++s)
        if (base[s] >= 0) pl.perm_of[s] = (int32_t)(std::find(bases.begin(), bases.end(), base[s]) - bases.begin());

    // ---- pairs ----------------------------------------------------------------------------------
    pl.hp.clear(); pl.owner.clear(); pl.nout = 0;
    for (size_t k = 0; k < pr.size(); ++k) {
        const int32_t q = pr[k][0], p = pr[k][1];
        const int64_t nq = sets[(size_t)q].n, np = sets[(size_t)p].n;
        if (nq == 0 || np == 0) continue;
        pl.hp.push_back(NnPair{(int32_t)pl.soff[(size_t)q], (int32_t)nq, (int32_t)pl.soff[(size_t)p], (int32_t)np, (int32_t)pl.nout,
                                pl.perm_of[(size_t)q] >= 0 ? (int32_t)pl.perm_off[(size_t)pl.perm_of[(size_t)q]] : -1});
        pl.owner.push_back((int)k);
        pl.nout += nq;
    }
    if (pl.npts() > (int64_t)1 << 30 || pl.nout > (int64_t)1 << 30)
        return set_error(MM_ERR_TOO_LARGE, std::string(what) + ": batch exceeds 2^30 points");
    pl.goff.assign(S + 1, 0);
    for (size_t s = 0; s < S; ++s) pl.goff[s + 1] = pl.goff[s] + (sets[s].n + pl.qpb - 1) / pl.qpb;
    pl.box.assign((size_t)pl.goff.back(), Box3{});
    return MM_OK;
}

// The boxes of set si's groups of qpb staged points; where dx != nullptr, also its staged coordinates (dx[j] = point
// j in staged order).  Derived sets are boxed from Set3::at, the arithmetic k_nn3_morph repeats on the device.
void nn_plan_stage_set(const std::vector<Set3>& sets, NnPlan& pl, size_t si, double* dx, double* dy, double* dz)
{
    const Set3& st = sets[si];
    const int32_t* pm = pl.perm_of[si] >= 0 ? pl.perms[(size_t)pl.perm_of[si]].data() : nullptr;
    for (int64_t g0 = 0, g = pl.goff[si]; g0 < st.n; g0 += pl.qpb, ++g) {
        Box3& b = pl.box[(size_t)g] = Box3{};
        for (int64_t j = g0; j < std::min<int64_t>(st.n, g0 + pl.qpb); ++j) {
            const int64_t i = pm ? (int64_t)pm[j] : j;
            const double v[3] = {st.at(i, 0), st.at(i, 1), st.at(i, 2)};
            if (dx) { dx[j] = v[0]; dy[j] = v[1]; dz[j] = v[2]; }
            b.add(v);
        }
    }
}

// lb2 of query block qb of set q against chunk c of set p: a chunk's box is the union of its groups', so the smallest
// of their bounds (mm_prune.h, box_lb2; the points lie in their boxes exactly: no slack)
inline double chunk_lb2(const NnPlan& pl, int32_t q, int64_t qb, int32_t p, int64_t c, int gpc)
{
    const Box3& bq = pl.box[(size_t)(pl.goff[(size_t)q] + qb)];
    double lb2 = DBL_MAX;
    for (int64_t g = c * gpc; g < std::min<int64_t>((c + 1) * gpc, pl.goff[(size_t)p + 1] - pl.goff[(size_t)p]); ++g)
        lb2 = std::min(lb2, box_lb2(bq, pl.box[(size_t)(pl.goff[(size_t)p] + g)], 0.0));
    return lb2;
}

// Device pair i's items of k_nn3_min: pass A (wa) runs for every query block the chunk with the smallest lb2, pass B
// (wb) every other chunk with its lb2.  Pairs that are not both sorted, or that have at most 2 chunks, scan everything
// in pass A, span chunks per item.
void nn_plan_min_items(const NnPlan& pl, const std::vector<std::array<int32_t, 2>>& pr, size_t i, std::vector<NnWork>& wa,
                       std::vector<NnWork>& wb)
{
    const int qpb = pl.qpb, ch = pl.ch, gpc = ch / qpb;   // groups per chunk
    const int32_t q = pr[(size_t)pl.owner[i]][0], p = pr[(size_t)pl.owner[i]][1];
    const int64_t nq = pl.hp[i].nq, np = pl.hp[i].np;
    const int64_t n_chunks = (np + ch - 1) / ch;
    const bool prune = pl.perm_of[(size_t)q] >= 0 && pl.perm_of[(size_t)p] >= 0 && n_chunks > 2 && gpc >= 1 && ch % qpb == 0;
    if (!prune) {
        for (int64_t q0 = 0; q0 < nq; q0 += qpb)
            for (int64_t c0 = 0; c0 < np; c0 += (int64_t)pl.span * ch)
                wa.push_back(NnWork{(int32_t)i, (int32_t)q0, (int32_t)c0, pl.span, 0.0});
        return;
    }
    std::vector<std::pair<double, int32_t>> cand;
    for (int64_t q0 = 0, qb = 0; q0 < nq; q0 += qpb, ++qb) {
        nearest_first(n_chunks, [&](int64_t c) { return chunk_lb2(pl, q, qb, p, c, gpc); }, cand);
        wa.push_back(NnWork{(int32_t)i, (int32_t)q0, cand[0].second * ch, 1, 0.0});
        for (size_t c = 1; c < cand.size(); ++c)
            wb.push_back(NnWork{(int32_t)i, (int32_t)q0, cand[c].second * ch, 1, cand[c].first});
    }
}

// Device pair i's items of k_nn3_count: the (query block, chunk) combinations whose boxes come within r2
void nn_plan_count_items(const NnPlan& pl, const std::vector<std::array<int32_t, 2>>& pr, size_t i, double r2,
                         std::vector<NnWork>& w)
{
    const int qpb = pl.qpb, ch = pl.ch, gpc = std::max(1, ch / qpb);
    const int32_t q = pr[(size_t)pl.owner[i]][0], p = pr[(size_t)pl.owner[i]][1];
    const int64_t nq = pl.hp[i].nq, np = pl.hp[i].np, n_chunks = (np + ch - 1) / ch;
    for (int64_t q0 = 0, qb = 0; q0 < nq; q0 += qpb, ++qb)
        for (int64_t c = 0; c < n_chunks; ++c) {
            const double lb2 = chunk_lb2(pl, q, qb, p, c, gpc);
            if (lb2 <= r2) w.push_back(NnWork{(int32_t)i, (int32_t)q0, (int32_t)(c * ch), 1, lb2});
        }
}

// The staging both nearest-neighbour launches share, through the engine's two pinned buffers: the point pool (x, y, z
// planes, the permutations, then what the caller carves behind them) in host_pts; pairs and work lists in host_lvl,
// which also receives the results, so that nothing in host_pts moves.  dev_pts holds them in that order, outputs last.
struct NnStage {
    Carve cv;
    size_t o_x, o_y, o_z, o_perm, o_pairs = 0, o_work[2] = {0, 0}, n_work[2] = {0, 0}, in_bytes = 0, o_out = 0, o_out2 = 0;
    unsigned char *h = nullptr, *hl = nullptr, *d = nullptr;

    explicit NnStage(const NnPlan& pl)
        : o_x(cv.take((size_t)pl.npts() * 8)), o_y(cv.take((size_t)pl.npts() * 8)), o_z(cv.take((size_t)pl.npts() * 8)),
          o_perm(cv.take((size_t)pl.perm_off.back() * 4)) {}
    template <class T> T* dev(size_t off) const { return (T*)(d + off); }

    // Pins host_pts for everything carved so far and fills the group boxes of every set, the staged coordinates of the
    // sets that exist on the host (the device writes a derived set's) and the permutations; extra(k), k < n_extra, runs
    // on the same worker pool.
    template <class Extra>
    int points(Engine* e, const std::vector<Set3>& sets, NnPlan& pl, size_t n_extra, Extra extra)
    {
        if (const int rc = e->ensure(e->host_pts, cv.size(), true)) return rc;
        h = (unsigned char*)e->host_pts.p;
        double *hx = (double*)(h + o_x), *hy = (double*)(h + o_y), *hz = (double*)(h + o_z);
        const size_t S = sets.size();
        parallel_for((int)(S + n_extra), [&](int job) {
            const size_t si = (size_t)job;
            if (si >= S) return extra(si - S);
            nn_plan_stage_set(sets, pl, si, sets[si].unit ? nullptr : hx + pl.soff[si], hy + pl.soff[si], hz + pl.soff[si]);
        });
        for (size_t k = 0; k < pl.perms.size(); ++k)
            std::memcpy(h + o_perm + (size_t)pl.perm_off[k] * 4, pl.perms[k].data(), pl.perms[k].size() * 4);
        return MM_OK;
    }
    // Builds the work lists over the worker pool (items(i, w0, w1) appends device pair i's; each list is pair-major),
    // carves pairs, lists and the two outputs behind the points, sizes host_lvl and dev_pts, fills host_lvl.
    template <class Items>
    int work(Engine* e, const NnPlan& pl, Items items, const char* too_many, size_t out_bytes, size_t out2_bytes)
    {
        const size_t P = pl.hp.size();
        std::vector<std::vector<NnWork>> per[2] = {std::vector<std::vector<NnWork>>(P), std::vector<std::vector<NnWork>>(P)};
        { TraceTimer tt("nn: work lists");
        parallel_for((int)P, [&](int i) { items((size_t)i, per[0][(size_t)i], per[1][(size_t)i]); });
        }
        o_pairs = cv.take(P * sizeof(NnPair));
        for (int l = 0; l < 2; ++l) {
            for (const auto& v : per[l]) n_work[l] += v.size();
            o_work[l] = cv.take(n_work[l] * sizeof(NnWork));
        }
        if (n_work[0] + n_work[1] > (size_t)1 << 30) return set_error(MM_ERR_TOO_LARGE, too_many);
        in_bytes = cv.size();
        o_out = cv.take(out_bytes); o_out2 = cv.take(out2_bytes);
        if (const int rc = e->ensure(e->host_lvl, std::max(in_bytes - o_pairs, out_bytes), true)) return rc;
        if (const int rc = e->ensure(e->dev_pts, cv.size(), false)) return rc;
        hl = (unsigned char*)e->host_lvl.p; d = (unsigned char*)e->dev_pts.p;
        std::memcpy(hl, pl.hp.data(), P * sizeof(NnPair));
        for (int l = 0; l < 2; ++l) {
            NnWork* dst = (NnWork*)(hl + (o_work[l] - o_pairs));
            for (const auto& v : per[l]) dst = std::copy(v.begin(), v.end(), dst);
        }
        return MM_OK;
    }
    int send(Engine* e, bool pool = true) const   // the point pool (unless the caller sent its parts), then pairs and lists
    {
        if (pool) MM_TRY_HIP(hipMemcpyAsync(d, h, o_pairs, hipMemcpyHostToDevice, e->stream));
        MM_TRY_HIP(hipMemcpyAsync(d + o_pairs, hl, in_bytes - o_pairs, hipMemcpyHostToDevice, e->stream));
        return MM_OK;
    }
    int fetch(Engine* e, size_t off, size_t bytes) const   // device output at `off` into host_lvl; synchronises
    {
        MM_TRY_HIP(hipMemcpyAsync(hl, d + off, bytes, hipMemcpyDeviceToHost, e->stream));
        MM_TRY_HIP(hipStreamSynchronize(e->stream));
        return MM_OK;
    }
};

// Per-query minima of every pair (sets[q] against sets[p]); one upload, two launches, one download.
// view[k] = {pointer, count}: pair k's minima, in the query set's ORIGINAL order, inside the engine's pinned
// staging buffer (valid until the next call on this engine); pointer == nullptr means "all +inf" (an empty
// point set) or no queries.
// order_like: as nn_plan_pairs takes it.  Pruned or not, sorted or not, the results are the same bits.
struct MinView { const double* p; int64_t n; };

// sums (nullable): if given, only the per-pair sums of the minima (sequential, index order) come back
// -- sums[k] for pair k, NaN where the pair has no minima -- and view[k].p stays null.
int nn_batch_view(Engine* e, const std::vector<Set3>& sets, const std::vector<std::array<int32_t, 2>>& pr,
                  std::vector<MinView>& view, const std::vector<int32_t>* order_like = nullptr,
                  std::vector<double>* sums = nullptr)
{
    if (sums) sums->assign(pr.size(), NAN);
    view.assign(pr.size(), MinView{nullptr, 0});
    const size_t S = sets.size();
    TraceTimer tt_all("nn: batch total");
    NnPlan pl;
    int rc = nn_plan_pairs(sets, pr, order_like, "nn batch", pl);
    if (rc) return rc;
    for (size_t k = 0; k < pr.size(); ++k) view[k].n = sets[(size_t)pr[k][0]].n;   // fold(INFINITY, min) over an empty set: all +inf
    if (pl.hp.empty()) return MM_OK;
    const int64_t nout = pl.nout;
    // derived sets: only their boxes are computed here; their coordinates are produced on the device from
    // an auxiliary pool (base point, unit vector, flag per point; one entry per distinct base + order)
    struct Aux { const double* xyz; const double* unit; const uint8_t* has; int32_t perm; int64_t n, off; };
    std::vector<Aux> aux;
    std::vector<int32_t> aux_of(S, -1);
    int64_t naux = 0;
    for (size_t s = 0; s < S; ++s) {
        const Set3& st = sets[s];
        if (!st.unit || st.n == 0) continue;
        size_t k = 0;
        for (; k < aux.size(); ++k)
            if (aux[k].xyz == st.xyz && aux[k].unit == st.unit && aux[k].has == st.has && aux[k].perm == pl.perm_of[s] && aux[k].n == st.n) break;
        if (k == aux.size()) { aux.push_back(Aux{st.xyz, st.unit, st.has, pl.perm_of[s], st.n, naux}); naux += st.n; }
        aux_of[s] = (int32_t)k;
    }
    std::vector<NnMorph> morphs;
    for (size_t s = 0; s < S; ++s)
        if (aux_of[s] >= 0) morphs.push_back(NnMorph{(int32_t)pl.soff[s], (int32_t)sets[s].n, (int32_t)aux[(size_t)aux_of[s]].off, 0, sets[s].adj});
    NnStage st(pl);
    const size_t o_aux = st.cv.take((size_t)naux * 7 * 8), o_morph = st.cv.take(morphs.size() * sizeof(NnMorph));
    { TraceTimer tt("nn: stage points + boxes");
    rc = st.points(e, sets, pl, aux.size(), [&](size_t k) {   // one auxiliary pool entry: 7 planes of naux, bx by bz ux uy uz flag
        double* haux = (double*)(st.h + o_aux);
        const Aux& ax = aux[k];
        const int32_t* pm = ax.perm >= 0 ? pl.perms[(size_t)ax.perm].data() : nullptr;
        for (int64_t j = 0; j < ax.n; ++j) {
            const int64_t i = pm ? (int64_t)pm[j] : j;
            for (int a = 0; a < 3; ++a) {
                haux[(size_t)a * (size_t)naux + (size_t)(ax.off + j)] = ax.xyz[3 * i + a];
                haux[(size_t)(3 + a) * (size_t)naux + (size_t)(ax.off + j)] = ax.unit[3 * i + a];
            }
            haux[(size_t)6 * (size_t)naux + (size_t)(ax.off + j)] = ax.has[i] ? 1.0 : 0.0;
        }
    });
    if (rc) return rc;
    }
    if (!morphs.empty()) std::memcpy(st.h + o_morph, morphs.data(), morphs.size() * sizeof(NnMorph));

    // pass A and pass B lists (nn_plan_min_items), the minima and the per-pair sums behind them
    rc = st.work(e, pl, [&](size_t i, std::vector<NnWork>& wa, std::vector<NnWork>& wb) { nn_plan_min_items(pl, pr, i, wa, wb); },
                 "nn batch exceeds 2^30 work items", (size_t)nout * 8, pl.hp.size() * 8);
    if (rc) return rc;
    TraceTimer tt_dev("nn: copies + kernels");
    if (!morphs.empty()) {
        // only the sets that exist on the host travel; the derived ones are written by the device
        for (size_t s2 = 0; s2 < S; ++s2) {
            if (aux_of[s2] >= 0 || sets[s2].n == 0) continue;
            for (size_t o : {st.o_x + (size_t)pl.soff[s2] * 8, st.o_y + (size_t)pl.soff[s2] * 8, st.o_z + (size_t)pl.soff[s2] * 8})
                MM_TRY_HIP(hipMemcpyAsync(st.d + o, st.h + o, (size_t)sets[s2].n * 8, hipMemcpyHostToDevice, e->stream));
        }
        MM_TRY_HIP(hipMemcpyAsync(st.d + st.o_perm, st.h + st.o_perm, st.o_pairs - st.o_perm, hipMemcpyHostToDevice, e->stream));
        const hipError_t hm = launch_nn3_morph(st.dev<const NnMorph>(o_morph), (int)morphs.size(), st.dev<const double>(o_aux), naux,
                                               st.dev<double>(st.o_x), st.dev<double>(st.o_y), st.dev<double>(st.o_z), e->stream);
        if (hm != hipSuccess) return hip_error(hm, "morph launch");
    }
    if ((rc = st.send(e, morphs.empty()))) return rc;
    const NnPair* d_pairs = st.dev<const NnPair>(st.o_pairs);
    const hipError_t he = launch_nn3_min(d_pairs, st.dev<const NnWork>(st.o_work[0]), (int)st.n_work[0], st.dev<const NnWork>(st.o_work[1]),
                                         (int)st.n_work[1], st.dev<const double>(st.o_x), st.dev<const double>(st.o_y), st.dev<const double>(st.o_z),
                                         st.dev<const int32_t>(st.o_perm), st.dev<double>(st.o_out), nout, e->stream);
    if (he != hipSuccess) return hip_error(he, "nearest-neighbour launch");
    if (sums) {
        const hipError_t hs = launch_nn3_sums(d_pairs, (int)pl.hp.size(), st.dev<const double>(st.o_out), st.dev<double>(st.o_out2), e->stream);
        if (hs != hipSuccess) return hip_error(hs, "sum launch");
        if ((rc = st.fetch(e, st.o_out2, pl.hp.size() * 8))) return rc;
        for (size_t i = 0; i < pl.hp.size(); ++i) (*sums)[(size_t)pl.owner[i]] = ((const double*)st.hl)[i];
        return MM_OK;
    }
    if ((rc = st.fetch(e, st.o_out, (size_t)nout * 8))) return rc;
    const double* res = (const double*)st.hl;
    for (size_t i = 0; i < pl.hp.size(); ++i) view[(size_t)pl.owner[i]].p = res + pl.hp[i].out_off;
    return MM_OK;
}

int nn_batch(Engine* e, const std::vector<Set3>& sets, const std::vector<std::array<int32_t, 2>>& pr,
             std::vector<std::vector<double>>& out)
{
    std::vector<MinView> view;
    int rc = nn_batch_view(e, sets, pr, view);
    if (rc) return rc;
    out.assign(pr.size(), {});
    for (size_t k = 0; k < pr.size(); ++k) {
        if (view[k].p) out[k].assign(view[k].p, view[k].p + view[k].n);
        else out[k].assign((size_t)view[k].n, INFINITY);
    }
    return MM_OK;
}

// symmetric_nn_distance (:188-216) from the two vectors of minima
double symmetric_from_minima(const MinView& a_to_b, const MinView& b_to_a)
{
    if (a_to_b.n == 0 || b_to_a.n == 0) return INFINITY;                      // :189-191
    if (!a_to_b.p || !b_to_a.p) return INFINITY;                              // unreachable: both sets non-empty
    double sa = 0.0;
    for (int64_t i = 0; i < a_to_b.n; ++i) sa += a_to_b.p[i];                 // :193-200, index order
    const double avg_a = sa / (double)a_to_b.n;                              // :202
    double sb = 0.0;
    for (int64_t i = 0; i < b_to_a.n; ++i) sb += b_to_a.p[i];                 // :204-211
    const double avg_b = sb / (double)b_to_a.n;                              // :213
    return std::sqrt((avg_a + avg_b) / 2.0);                                  // :215
}

// the same from the two sums of minima (sequential folds done on the device)
double symmetric_from_sums(double sa, int64_t na, double sb, int64_t nb)
{
    if (na == 0 || nb == 0) return INFINITY;                                  // :189-191
    return std::sqrt((sa / (double)na + sb / (double)nb) / 2.0);              // :202, :213, :215
}

// unit vector from the closest centerline point to each point (:226-235); has[i] = 0 when the point sits
// on its centerline point (try_normalize(0.0) fails -> the point does not move)
void radial_units(const mm_clpoint* cl, int64_t ncl, const double* pts, int64_t n, std::vector<double>& unit,
                  std::vector<uint8_t>& has)
{
    unit.assign((size_t)n * 3, 0.0);
    has.assign((size_t)n, 0);
    constexpr int64_t kBlock = 256;
    parallel_for((int)((n + kBlock - 1) / kBlock), [&](int blk) {
        const int64_t i0 = (int64_t)blk * kBlock;
        for (int64_t i = i0; i < std::min(n, i0 + kBlock); ++i) {
            const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
            double best = DBL_MAX;                                            // :249-258
            int64_t kb = 0;
            for (int64_t k = 0; k < ncl; ++k) {
                const double dx = x - cl[k].x, dy = y - cl[k].y, dz = z - cl[k].z;
                const double d = dx * dx + dy * dy + dz * dz;
                if (d < best) { best = d; kb = k; }
            }
            const double vx = x - cl[kb].x, vy = y - cl[kb].y, vz = z - cl[kb].z;
            const double nn = std::sqrt(vx * vx + vy * vy + vz * vz);
            if (nn > 0.0) { unit[3 * i] = vx / nn; unit[3 * i + 1] = vy / nn; unit[3 * i + 2] = vz / nn; has[i] = 1; }
        }
    });
}

inline void morph(const double* pts, const std::vector<double>& unit, const std::vector<uint8_t>& has, int64_t n,
                  double adj, double* out)
{
    for (int64_t i = 0; i < n; ++i) {
        if (has[i]) {
            out[3 * i] = pts[3 * i] + unit[3 * i] * adj;                      // :236 p + unit * x
            out[3 * i + 1] = pts[3 * i + 1] + unit[3 * i + 1] * adj;
            out[3 * i + 2] = pts[3 * i + 2] + unit[3 * i + 2] * adj;
        } else { out[3 * i] = pts[3 * i]; out[3 * i + 1] = pts[3 * i + 1]; out[3 * i + 2] = pts[3 * i + 2]; }  // :239
    }
}

// the 41-step loop of :75-87 / :107-129: all scalings scored in one device batch
int scaling_search(Engine* e, const double* pts, int64_t n, const double* ref, int64_t nr, const mm_clpoint* cl,
                   int64_t ncl, double& best, double* all_dist)
{
    const double start = -2.0, end = 2.0, step = 0.1;
    const int steps = (int)std::round((end - start) / step);                  // :70-73
    best = DBL_MAX;
    double min_dist = DBL_MAX;
    std::vector<double> dist((size_t)steps + 1, INFINITY);
    if (n > 0 && nr > 0) {
        if (ncl <= 0) return set_error(MM_ERR_INVALID, "diameter search: empty centerline");
        std::vector<double> unit; std::vector<uint8_t> has;
        { TraceTimer tt("ccta: radial units"); radial_units(cl, ncl, pts, n, unit, has); }
        std::vector<Set3> sets;
        std::vector<std::array<int32_t, 2>> pr;
        sets.push_back(Set3{ref, nr});
        for (int i = 0; i <= steps; ++i) {
            const double x = start + (double)i * step;                        // :79
            sets.push_back(Set3{pts, n, unit.data(), has.data(), x});         // :80, computed where it is used
            pr.push_back({0, i + 1});                                         // reference -> moved
            pr.push_back({i + 1, 0});                                         // moved -> reference
        }
        // every morphed copy shares the spatial order of the first (points move by at most 2 mm)
        std::vector<int32_t> order_like(sets.size(), 1);
        order_like[0] = 0;
        std::vector<MinView> mins;
        std::vector<double> sums;   // the 82 sequential sums are taken on the device: 82 numbers come back, not 13 MB
        int rc = nn_batch_view(e, sets, pr, mins, &order_like, &sums);
        if (rc) return rc;
        for (int i = 0; i <= steps; ++i)
            dist[(size_t)i] = symmetric_from_sums(sums[2 * (size_t)i], mins[2 * (size_t)i].n, sums[2 * (size_t)i + 1], mins[2 * (size_t)i + 1].n);  // :81
    }
    for (int i = 0; i <= steps; ++i) {
        if (all_dist) all_dist[i] = dist[(size_t)i];
        if (dist[(size_t)i] < min_dist) { min_dist = dist[(size_t)i]; best = start + (double)i * step; }  // :82-85
    }
    return MM_OK;
}

// find_region_points (:133-183)
int region_points(Engine* e, const double* an, int64_t n, const double* ref, int64_t nr, int64_t n_points,
                  std::vector<double>& selected, std::vector<double>& remaining)
{
    selected.clear();
    if (n == 0 || nr == 0 || n_points == 0) { remaining.assign(an, an + 3 * n); return MM_OK; }  // :138-140
    std::vector<std::vector<double>> mins;
    int rc = nn_batch(e, {Set3{an, n}, Set3{ref, nr}}, {{0, 1}}, mins);      // :142-152
    if (rc) return rc;
    const std::vector<double>& d = mins[0];
    std::vector<int64_t> order((size_t)n);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::sort(order.begin(), order.end(), [&d](int64_t a, int64_t b) {       // :154-158
        if (d[(size_t)a] < d[(size_t)b]) return true;
        if (d[(size_t)a] > d[(size_t)b]) return false;
        return a < b;
    });
    const int64_t take = std::min(n_points, n);                               // :160
    std::vector<uint8_t> sel((size_t)n, 0);
    selected.reserve((size_t)take * 3);
    for (int64_t k = 0; k < take; ++k) {
        const int64_t i = order[(size_t)k];
        sel[(size_t)i] = 1;
        selected.insert(selected.end(), an + 3 * i, an + 3 * i + 3);          // :165-168
    }
    remaining.clear();
    remaining.reserve((size_t)(n - take) * 3);
    for (int64_t i = 0; i < n; ++i) if (!sel[(size_t)i]) remaining.insert(remaining.end(), an + 3 * i, an + 3 * i + 3);  // :170-180
    return MM_OK;
}

// ---- neighbour counts within a radius (clean_up_non_section_points, scale_coronary.rs:342-409) ------------
// counts[k][i] = #{p in sets[pr[k][1]] : |q_i - p|^2 <= r2} for every query q_i of sets[pr[k][0]], exact f64 on
// the device (k_nn3_count) over the items of nn_plan_count_items; a count does not depend on the order.
int radius_counts(Engine* e, const std::vector<Set3>& sets, const std::vector<std::array<int32_t, 2>>& pr, double r2,
                  std::vector<std::vector<uint32_t>>& counts)
{
    counts.assign(pr.size(), {});
    NnPlan pl;
    int rc = nn_plan_pairs(sets, pr, nullptr, "radius counts", pl);
    if (rc) return rc;
    for (size_t k = 0; k < pr.size(); ++k) counts[k].assign((size_t)sets[(size_t)pr[k][0]].n, 0u);
    if (pl.hp.empty()) return MM_OK;
    NnStage st(pl);
    if ((rc = st.points(e, sets, pl, 0, [](size_t) {}))) return rc;
    rc = st.work(e, pl, [&](size_t i, std::vector<NnWork>& w, std::vector<NnWork>&) { nn_plan_count_items(pl, pr, i, r2, w); },
                 "radius counts: too many work items", (size_t)pl.nout * 4, 0);
    if (rc || (rc = st.send(e))) return rc;
    const hipError_t he = launch_nn3_count(st.dev<const NnPair>(st.o_pairs), st.dev<const NnWork>(st.o_work[0]), (int)st.n_work[0],
                                           st.dev<const double>(st.o_x), st.dev<const double>(st.o_y), st.dev<const double>(st.o_z),
                                           st.dev<const int32_t>(st.o_perm), r2, st.dev<unsigned int>(st.o_out), pl.nout, e->stream);
    if (he != hipSuccess) return hip_error(he, "radius-count launch");
    if ((rc = st.fetch(e, st.o_out, (size_t)pl.nout * 4))) return rc;
    const uint32_t* res = (const uint32_t*)st.hl;
    for (size_t i = 0; i < pl.hp.size(); ++i)
        std::memcpy(counts[(size_t)pl.owner[i]].data(), res + pl.hp[i].out_off, (size_t)pl.hp[i].nq * 4);
    return MM_OK;
}

// clean_up_non_section_points (:342-409).  to_ref[i] = 1: point i of `cleanup` joins the reference set (appended
// in input order), 0: it stays.
int clean_up_points(Engine* e, const double* cleanup, int64_t nc, const double* reference, int64_t nr, double radius,
                    double min_ratio, std::vector<uint8_t>& to_ref)
{
    to_ref.assign((size_t)nc, 0);
    if (nc == 0) return MM_OK;                                                        // :353-355
    const double r2 = radius * radius;                                                // :348
    std::vector<std::vector<uint32_t>> cnt;
    int rc = radius_counts(e, {Set3{cleanup, nc}, Set3{reference, nr}}, {{0, 1}, {0, 0}}, r2, cnt);
    if (rc) return rc;
    for (int64_t i = 0; i < nc; ++i) {
        const uint64_t ref_n = cnt[0][(size_t)i];                                     // :375-377
        const uint64_t self_n = cnt[1][(size_t)i] > 0 ? cnt[1][(size_t)i] - 1 : 0;    // :381-384 saturating_sub(1)
        const uint64_t total = ref_n + self_n;
        if (total > 0) {                                                              // :388-400
            const double ratio = (double)ref_n / (double)total;
            to_ref[(size_t)i] = ratio >= min_ratio ? 1 : 0;
        }
    }
    return MM_OK;
}


// ---- mesh labelling (src/ccta/adjust_mesh/label_coronary.rs) -----------------------------------------------------

// Centerline::mean_spacing (centerline.rs:304-320): mean distance of consecutive points of the first branch (the
// points before the first change of branch id), 1.0 below two points; summed in index order
double cl_mean_spacing(const mm_clpoint* cl, int64_t n)
{
    if (n <= 0) return 1.0;
    int64_t end = 1;
    while (end < n && cl[end].branch_id == cl[0].branch_id) ++end;
    if (end < 2) return 1.0;
    double s = 0.0;
    for (int64_t i = 1; i < end; ++i) {
        const double dx = cl[i - 1].x - cl[i].x, dy = cl[i - 1].y - cl[i].y, dz = cl[i - 1].z - cl[i].z;
        s += std::sqrt(dx * dx + dy * dy + dz * dz);
    }
    return s / (double)(end - 1);
}

// Rust's saturating `x as usize`: NaN and negatives -> 0, beyond the range -> the maximum
uint64_t sat_usize(double x)
{
    if (!(x > 0.0)) return 0;
    if (x >= 18446744073709551616.0) return UINT64_MAX;
    return (uint64_t)x;
}

std::vector<double> cl_xyz(const mm_clpoint* cl, int64_t n)
{
    std::vector<double> v((size_t)n * 3);
    for (int64_t i = 0; i < n; ++i) { v[3 * i] = cl[i].x; v[3 * i + 1] = cl[i].y; v[3 * i + 2] = cl[i].z; }
    return v;
}

// remove_occluded_points_ray_triangle_rust (:70-197).  removed[i] = 1: point i goes; excluded[f] = 1: face f is the
// closest hit of some ray that hits >= 3 faces.  Rays on the device (mm_ray_kernels.hip), the vertex pass on the
// radius-count path.
int occluded_points(Engine* e, const mm_clpoint* cc, int64_t ncc, const mm_clpoint* ca, int64_t nca, double range_mm,
                    const double* pts, int64_t n, const double* tri, int64_t nf, double step_mm,
                    std::vector<uint8_t>& removed, std::vector<uint8_t>& excluded)
{
    removed.assign((size_t)n, 0);
    excluded.assign((size_t)nf, 0);
    if (n == 0 || nf == 0 || nca == 0) return MM_OK;                                   // :78-80; no aortic point, no ray
    const double spacing = (cl_mean_spacing(ca, nca) + cl_mean_spacing(cc, ncc)) / 2.0;   // :85
    const uint64_t step = sat_usize(std::ceil(step_mm / spacing));                         // :86
    const uint64_t range = sat_usize(std::ceil(range_mm / spacing));                       // :89
    if (step == 0) return set_error(MM_ERR_INVALID, "mm_occluded_points: step_size_mm / spacing gives a step of 0 points");
    // the coronary points of .take(range).step_by(step) (:104-108)
    std::vector<int64_t> cor;
    const uint64_t lim = std::min<uint64_t>(range, (uint64_t)ncc);
    for (uint64_t i = 0; i < lim;) {
        cor.push_back((int64_t)i);
        if (step >= lim - i) break;
        i += step;
    }
    const int64_t R = nca * (int64_t)cor.size();
    if (R == 0) return MM_OK;
    const int ch = ray_chunk_faces(), rb = ray_block_rays();
    const int64_t n_chunks = (nf + ch - 1) / ch, n_rblk = (R + rb - 1) / rb;
    const size_t part_bytes = sizeof(RayPartial) * (size_t)R * (size_t)n_chunks;
    if (R > INT32_MAX / 8 || nf > INT32_MAX / 16 || n_chunks * n_rblk > INT32_MAX || part_bytes > ((size_t)4 << 30))
        return set_error(MM_ERR_TOO_LARGE, "mm_occluded_points: too many rays x faces for one pass");
    StagedPass sp;
    const size_t o_ray = sp.in.take((size_t)R * 6 * 8), o_tri = sp.in.take((size_t)nf * 9 * 8);
    const size_t o_cl = sp.out.take((size_t)R * 4), o_part = sp.scratch.take(part_bytes);
    int rc = sp.reserve(e);
    if (rc) return rc;
    double* hr = sp.host<double>(o_ray);
    double* ht = sp.host<double>(o_tri);
    const int64_t nc = (int64_t)cor.size();
    for (int64_t a = 0; a < nca; ++a)
        for (int64_t k = 0; k < nc; ++k) {
            const int64_t r = a * nc + k;
            const mm_clpoint& o = ca[a];
            const mm_clpoint& c = cc[cor[(size_t)k]];
            hr[r] = o.x; hr[R + r] = o.y; hr[2 * R + r] = o.z;
            hr[3 * R + r] = c.x - o.x; hr[4 * R + r] = c.y - o.y; hr[5 * R + r] = c.z - o.z;        // :117 coronary - aorta
        }
    for (int64_t f = 0; f < nf; ++f) {
        const double* t = tri + 9 * f;
        for (int ax = 0; ax < 3; ++ax) {
            ht[(size_t)ax * nf + f] = t[ax];                                                         // v0
            ht[(size_t)(3 + ax) * nf + f] = t[3 + ax] - t[ax];                                       // edge1 = v1 - v0 (:38)
            ht[(size_t)(6 + ax) * nf + f] = t[6 + ax] - t[ax];                                       // edge2 = v2 - v0 (:39)
        }
    }
    rc = sp.run((double)R * (double)nf, "ray-triangle launch", [&] {
        return launch_ray_tri(sp.dev_in<double>(o_ray), (int)R, sp.dev_in<double>(o_tri), (int)nf,
                              sp.dev_scratch<RayPartial>(o_part), sp.dev_out<int32_t>(o_cl), e->stream);
    });
    if (rc) return rc;
    const int32_t* closest = sp.host<int32_t>(o_cl);
    for (int64_t r = 0; r < R; ++r)
        if (closest[r] >= 0) excluded[(size_t)closest[r]] = 1;
    // :143-183 a point goes iff a vertex of an excluded face lies within squared distance 0.5
    std::vector<double> ev;
    for (int64_t f = 0; f < nf; ++f)
        if (excluded[(size_t)f]) ev.insert(ev.end(), tri + 9 * f, tri + 9 * f + 9);
    if (ev.empty()) return MM_OK;
    std::vector<std::vector<uint32_t>> cnt;
    if ((rc = radius_counts(e, {Set3{pts, n}, Set3{ev.data(), (int64_t)(ev.size() / 3)}}, {{0, 1}}, 0.5, cnt))) return rc;
    for (int64_t i = 0; i < n; ++i) removed[(size_t)i] = cnt[0][(size_t)i] > 0 ? 1 : 0;
    return MM_OK;
}

// exact bit-pattern key of a coordinate (bits_key, :293)
struct BitsKey {
    uint64_t x, y, z;
    bool operator==(const BitsKey& o) const { return x == o.x && y == o.y && z == o.z; }
};
struct BitsHash {
    size_t operator()(const BitsKey& k) const
    {
        uint64_t h = k.x * 0x9E3779B97F4A7C15ull;
        h ^= k.y + 0x7F4A7C159E3779B9ull + (h << 6) + (h >> 2);
        h ^= k.z + 0x94D049BB133111EBull + (h << 6) + (h >> 2);
        return (size_t)h;
    }
};
inline BitsKey bits_key(const double* p)
{
    BitsKey k;
    std::memcpy(&k.x, p, 8); std::memcpy(&k.y, p + 1, 8); std::memcpy(&k.z, p + 2, 8);
    return k;
}

// connected_components (label_coronary.rs:428-455) of the vertices v < nv with in(v), on the mesh adjacency restricted
// to them.  Components are found from their smallest vertex upwards; comp[v] = the component of v (-1 outside).
template <class In>
void components(const Adjacency& adj, int64_t nv, In in, std::vector<int64_t>& comp,
                std::vector<std::vector<int64_t>>& comps)
{
    comp.assign((size_t)nv, -1);
    comps.clear();
    for (int64_t s = 0; s < nv; ++s) {
        if (!in(s) || comp[(size_t)s] >= 0) continue;
        const int64_t c = (int64_t)comps.size();
        comps.emplace_back();
        std::vector<int64_t> stack{s};
        comp[(size_t)s] = c;
        while (!stack.empty()) {
            const int64_t v = stack.back();
            stack.pop_back();
            comps.back().push_back(v);
            for (const int64_t* p = adj.begin(v); p != adj.end(v); ++p)
                if (in(*p) && comp[(size_t)*p] < 0) { comp[(size_t)*p] = c; stack.push_back(*p); }
        }
    }
}

// The largest of the components (comps non-empty); among equally large ones the first found, i.e. the one holding the
// smallest vertex index: the reference picks one of them in HashSet order, so this is one of the outcomes it can
// produce.
size_t largest_component(const std::vector<std::vector<int64_t>>& comps)
{
    size_t largest = 0;
    for (size_t c = 1; c < comps.size(); ++c)
        if (comps[c].size() > comps[largest].size()) largest = c;
    return largest;
}

// reclassify_minority_components (:485-544): every component of `subject` but the largest moves to a target label
// that holds more than 70 % of its boundary.
void reclassify_minority(const Adjacency& adj, const std::vector<uint8_t>& labels, std::vector<uint8_t>& out,
                         uint8_t subject, const std::vector<uint8_t>& targets)
{
    const int64_t nv = (int64_t)labels.size();
    std::vector<int64_t> comp;
    std::vector<std::vector<int64_t>> comps;
    components(adj, nv, [&](int64_t v) { return labels[(size_t)v] == subject; }, comp, comps);
    if (comps.empty()) return;
    const size_t largest = largest_component(comps);
    std::vector<int64_t> mark((size_t)nv, -1);
    for (size_t c = 0; c < comps.size(); ++c) {
        if (c == largest) continue;
        int64_t bsize = 0;                                                            // component_boundary (:463-476)
        std::vector<int64_t> tcnt(targets.size(), 0);
        for (const int64_t v : comps[c])
            for (const int64_t* p = adj.begin(v); p != adj.end(v); ++p)
                if (comp[(size_t)*p] != (int64_t)c && mark[(size_t)*p] != (int64_t)c) {
                    mark[(size_t)*p] = (int64_t)c;
                    ++bsize;
                    for (size_t k = 0; k < targets.size(); ++k) tcnt[k] += labels[(size_t)*p] == targets[k] ? 1 : 0;
                }
        if (bsize == 0) continue;
        for (size_t k = 0; k < targets.size(); ++k)
            if ((double)tcnt[k] > (double)bsize * 0.7) {                                // :533-541, first target wins
                for (const int64_t v : comps[c]) out[(size_t)v] = targets[k];
                break;
            }
    }
}

// restore_removed_by_propagation (:546-631): round 0 tallies each removed vertex's real neighbours; every later round
// the vertices decided in the previous round vote for their undecided removed neighbours, all votes of a round applied
// together; a strict majority decides, ties stay undecided (and removed)
void restore_removed(const Adjacency& adj, const std::vector<uint8_t>& labels, std::vector<uint8_t>& out,
                     uint8_t removed_label, uint8_t target)
{
    const int64_t nv = (int64_t)labels.size();
    std::vector<int64_t> tc((size_t)nv, 0), oc((size_t)nv, 0), dt((size_t)nv, 0), dn((size_t)nv, 0);
    std::vector<int8_t> dec((size_t)nv, -1);
    std::vector<uint8_t> touched((size_t)nv, 0);
    std::vector<int64_t> frontier;
    for (int64_t v = 0; v < nv; ++v) {
        if (labels[(size_t)v] != removed_label) continue;
        for (const int64_t* p = adj.begin(v); p != adj.end(v); ++p) {
            const uint8_t l = labels[(size_t)*p];
            if (l == removed_label) continue;
            if (l == target) ++tc[(size_t)v]; else ++oc[(size_t)v];
        }
        if (tc[(size_t)v] != oc[(size_t)v]) { dec[(size_t)v] = tc[(size_t)v] > oc[(size_t)v] ? 1 : 0; frontier.push_back(v); }
    }
    while (!frontier.empty()) {
        std::vector<int64_t> hit;
        for (const int64_t v : frontier) {
            const bool is_t = dec[(size_t)v] == 1;
            for (const int64_t* p = adj.begin(v); p != adj.end(v); ++p) {
                const int64_t u = *p;
                if (labels[(size_t)u] != removed_label || dec[(size_t)u] >= 0) continue;
                if (!touched[(size_t)u]) { touched[(size_t)u] = 1; hit.push_back(u); }
                if (is_t) ++dt[(size_t)u]; else ++dn[(size_t)u];
            }
        }
        std::vector<int64_t> next;
        for (const int64_t u : hit) {
            tc[(size_t)u] += dt[(size_t)u]; oc[(size_t)u] += dn[(size_t)u];
            dt[(size_t)u] = dn[(size_t)u] = 0; touched[(size_t)u] = 0;
            if (tc[(size_t)u] != oc[(size_t)u]) { dec[(size_t)u] = tc[(size_t)u] > oc[(size_t)u] ? 1 : 0; next.push_back(u); }
        }
        frontier.swap(next);
    }
    for (int64_t v = 0; v < nv; ++v)
        if (dec[(size_t)v] == 1) out[(size_t)v] = target;
}


// ---- centerline morphing (scale_coronary.rs:218-260) on the device ----------------------------------------------

// every point of every job moved about its nearest centerline point of that job (k_cl_morph); every job with points
// has a centerline point (checked by the caller)
int cl_morph(Engine* e, int n_jobs, const mm_clpoint* cl, const int64_t* cl_off, const double* pts,
             const int64_t* pt_off, const double* adj, double* out, int32_t* nearest)
{
    const int64_t NP = pt_off[n_jobs], NC = cl_off[n_jobs];
    if (NP == 0) return MM_OK;
    if (NP > INT32_MAX / 4 || NC > INT32_MAX / 4)
        return set_error(MM_ERR_TOO_LARGE, "centerline morphing: too many points for one pass");
    std::vector<MorphJob> jobs((size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j)
        jobs[(size_t)j] = MorphJob{(int32_t)pt_off[j], (int32_t)(pt_off[j + 1] - pt_off[j]), (int32_t)cl_off[j],
                                   (int32_t)(cl_off[j + 1] - cl_off[j]), adj[j]};
    auto fill_cl = [&](double* hc) {
        for (int64_t k = 0; k < NC; ++k) { hc[3 * k] = cl[k].x; hc[3 * k + 1] = cl[k].y; hc[3 * k + 2] = cl[k].z; }
    };
    return nearest_pass(e, jobs, pt_off, pts, cl_off, 3, fill_cl, morph_block_points(), launch_cl_morph,
                        "centerline morphing launch", nearest, out);
}

}  // namespace
}  // namespace mm

using namespace mm;

extern "C" {

int mm_nn_min_sq_batch(mm_engine* h, int n_sets, const int64_t* set_off, const double* xyz, int n_pairs,
                       const int32_t* q_set, const int32_t* p_set, const int64_t* out_off, double* out)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (n_sets < 0 || n_pairs < 0 || (n_sets > 0 && !set_off) || (n_pairs > 0 && (!q_set || !p_set || !out_off || !out)))
        return set_error(MM_ERR_INVALID, "mm_nn_min_sq_batch: bad arguments");
    std::vector<Set3> sets((size_t)n_sets);
    for (int s = 0; s < n_sets; ++s) {
        const int64_t n = set_off[s + 1] - set_off[s];
        if (n < 0 || n > INT32_MAX || (n > 0 && !xyz)) return set_error(MM_ERR_INVALID, "bad set extent");
        sets[(size_t)s] = Set3{xyz ? xyz + 3 * set_off[s] : nullptr, n};
    }
    std::vector<std::array<int32_t, 2>> pr((size_t)n_pairs);
    for (int k = 0; k < n_pairs; ++k) {
        pr[(size_t)k] = {q_set[k], p_set[k]};
        if (q_set[k] < 0 || q_set[k] >= n_sets || p_set[k] < 0 || p_set[k] >= n_sets)
            return set_error(MM_ERR_INVALID, "mm_nn_min_sq_batch: set index out of range");
        if (out_off[k + 1] - out_off[k] != sets[(size_t)q_set[k]].n)
            return set_error(MM_ERR_INVALID, "mm_nn_min_sq_batch: out_off does not match the query set sizes");
    }
    std::vector<std::vector<double>> mins;
    if ((rc = nn_batch(e, sets, pr, mins))) return rc;
    for (int k = 0; k < n_pairs; ++k)
        if (!mins[(size_t)k].empty()) std::memcpy(out + out_off[k], mins[(size_t)k].data(), mins[(size_t)k].size() * 8);
    return MM_OK;
}

// The work lists of one nearest-neighbour batch and of one radius count, as the launch paths build them, without an
// engine.  A test hook for the pruning claims; nothing in the product calls it.
int mm_nn_plan(int n_sets, const int64_t* set_off, const double* xyz, const double* unit, const uint8_t* has,
               const uint8_t* derived, const double* adj, const int32_t* order_like, int n_pairs, const int32_t* q_set,
               const int32_t* p_set, double r2, int32_t* perm, int64_t* info, int32_t* items, double* item_lb2, int64_t cap)
{
    if (n_sets < 0 || n_pairs < 0 || cap < 0 || !info || (n_sets > 0 && !set_off) || (n_pairs > 0 && (!q_set || !p_set)) ||
        (cap > 0 && (!items || !item_lb2)))
        return set_error(MM_ERR_INVALID, "mm_nn_plan: bad arguments");
    std::vector<Set3> sets((size_t)n_sets);
    for (int s = 0; s < n_sets; ++s) {
        const int64_t n = set_off[s + 1] - set_off[s];
        if (set_off[s] < 0 || n < 0 || n > INT32_MAX || (n > 0 && !xyz)) return set_error(MM_ERR_INVALID, "mm_nn_plan: bad set extent");
        sets[(size_t)s] = Set3{xyz ? xyz + 3 * set_off[s] : nullptr, n};
        if (derived && derived[s] && n > 0) {
            if (!unit || !has || !adj) return set_error(MM_ERR_INVALID, "mm_nn_plan: a derived set needs unit, has and adj");
            sets[(size_t)s] = Set3{xyz + 3 * set_off[s], n, unit + 3 * set_off[s], has + set_off[s], adj[s]};
        }
    }
    if (n_sets > 0 && set_off[n_sets] > 0 && !perm) return set_error(MM_ERR_INVALID, "mm_nn_plan: perm == NULL");
    std::vector<std::array<int32_t, 2>> pr((size_t)n_pairs);
    for (int k = 0; k < n_pairs; ++k) pr[(size_t)k] = {q_set[k], p_set[k]};
    std::vector<int32_t> ol;
    if (order_like) ol.assign(order_like, order_like + n_sets);
    NnPlan pl;
    int rc = nn_plan_pairs(sets, pr, order_like ? &ol : nullptr, "mm_nn_plan", pl);
    if (rc) return rc;
    for (size_t s = 0; s < sets.size(); ++s) {
        nn_plan_stage_set(sets, pl, s, nullptr, nullptr, nullptr);
        int32_t* dst = perm + set_off[s];
        if (pl.perm_of[s] >= 0) std::memcpy(dst, pl.perms[(size_t)pl.perm_of[s]].data(), (size_t)sets[s].n * 4);
        else for (int64_t j = 0; j < sets[s].n; ++j) dst[j] = (int32_t)j;
    }
    std::vector<NnWork> lists[3];   // pass A, pass B, radius count
    for (size_t i = 0; i < pl.hp.size(); ++i) {
        nn_plan_min_items(pl, pr, i, lists[0], lists[1]);
        nn_plan_count_items(pl, pr, i, r2, lists[2]);
    }
    int64_t k = 0;
    for (int l = 0; l < 3; ++l) {
        info[l] = (int64_t)lists[l].size();
        for (const NnWork& w : lists[l]) {
            if (k < cap) {
                int32_t* it = items + 5 * k;
                it[0] = l; it[1] = pl.owner[(size_t)w.pair]; it[2] = w.q0; it[3] = w.c0; it[4] = w.n_chunks;
                item_lb2[k] = w.lb2;
            }
            ++k;
        }
    }
    info[3] = pl.qpb; info[4] = pl.ch; info[5] = pl.span;
    return MM_OK;
}

int mm_symmetric_nn_distance(mm_engine* h, const double* a, int64_t na, const double* b, int64_t nb, double* out)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (!out || na < 0 || nb < 0 || (na > 0 && !a) || (nb > 0 && !b)) return set_error(MM_ERR_INVALID, "mm_symmetric_nn_distance: bad arguments");
    if (na == 0 || nb == 0) { *out = INFINITY; return MM_OK; }
    std::vector<MinView> mins;
    if ((rc = nn_batch_view(e, {Set3{a, na}, Set3{b, nb}}, {{0, 1}, {1, 0}}, mins))) return rc;
    *out = symmetric_from_minima(mins[0], mins[1]);
    return MM_OK;
}

int mm_diameter_morphing(const mm_clpoint* cl, int64_t ncl, const double* pts, int64_t n, double adj, double* out)
{
    if (n < 0 || (n > 0 && (!pts || !out))) return set_error(MM_ERR_INVALID, "mm_diameter_morphing: bad arguments");
    if (n > 0 && (ncl <= 0 || !cl)) return set_error(MM_ERR_INVALID, "mm_diameter_morphing: empty centerline");  // points[0] panics
    std::vector<double> unit; std::vector<uint8_t> has;
    radial_units(cl, ncl, pts, n, unit, has);
    morph(pts, unit, has, n, adj, out);
    return MM_OK;
}

int64_t mm_find_region_points(mm_engine* h, const double* an, int64_t n, const double* ref, int64_t nr,
                              int64_t n_points, double* selected, double* remaining)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (n < 0 || nr < 0 || n_points < 0 || (n > 0 && (!an || !selected || !remaining)) || (nr > 0 && !ref))
        return set_error(MM_ERR_INVALID, "mm_find_region_points: bad arguments");
    std::vector<double> sel, rem;
    if ((rc = region_points(e, an, n, ref, nr, n_points, sel, rem))) return rc;
    if (!sel.empty()) std::memcpy(selected, sel.data(), sel.size() * 8);
    if (!rem.empty()) std::memcpy(remaining, rem.data(), rem.size() * 8);
    return (int64_t)(sel.size() / 3);
}

int mm_aortic_diameter_optimization(mm_engine* h, const double* intramural, int64_t ni, const double* reference,
                                    int64_t nr, const mm_clpoint* cl, int64_t ncl, double* best, double* all_dist)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (!best || ni < 0 || nr < 0 || (ni > 0 && !intramural) || (nr > 0 && !reference))
        return set_error(MM_ERR_INVALID, "mm_aortic_diameter_optimization: bad arguments");
    return scaling_search(e, intramural, ni, reference, nr, cl, ncl, *best, all_dist);
}

int mm_diameter_optimization(mm_engine* h, const double* an, int64_t n, int64_t n_prox, int64_t n_dist,
                             const mm_clpoint* cl, int64_t ncl, const double* pref, int64_t npr, const double* dref,
                             int64_t ndr, double* prox_best, double* dist_best)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (!prox_best || !dist_best || n < 0 || npr < 0 || ndr < 0 || n_prox < 0 || n_dist < 0 || (n > 0 && !an) ||
        (npr > 0 && !pref) || (ndr > 0 && !dref))
        return set_error(MM_ERR_INVALID, "mm_diameter_optimization: bad arguments");
    std::vector<double> prox, rest, dist, rest2;
    if ((rc = region_points(e, an, n, pref, npr, n_prox, prox, rest))) return rc;                    // :98-99
    if ((rc = region_points(e, rest.data(), (int64_t)(rest.size() / 3), dref, ndr, n_dist, dist, rest2))) return rc;  // :100
    if ((rc = scaling_search(e, prox.data(), (int64_t)(prox.size() / 3), pref, npr, cl, ncl, *prox_best, nullptr))) return rc;  // :112-120
    return scaling_search(e, dist.data(), (int64_t)(dist.size() / 3), dref, ndr, cl, ncl, *dist_best, nullptr);                // :121-129
}

int mm_wall_diameter_optimization(const mm_clpoint* cl, int64_t ncl, const double ref[3], const double* aortic,
                                  int64_t na, double* out)
{
    if (!out || !ref || ncl < 0 || na < 0 || (ncl > 0 && !cl) || (na > 0 && !aortic))
        return set_error(MM_ERR_INVALID, "mm_wall_diameter_optimization: bad arguments");
    *out = 0.0;
    if (ncl == 0 || na == 0) return MM_OK;                                                           // :13-15
    int64_t kc = 0, ka = 0;
    double bc = INFINITY, ba = INFINITY;                                                             // min_by: first minimum (:17-37)
    for (int64_t k = 0; k < ncl; ++k) {
        const double dx = cl[k].x - ref[0], dy = cl[k].y - ref[1], dz = cl[k].z - ref[2];
        const double d = dx * dx + dy * dy + dz * dz;
        if (d < bc) { bc = d; kc = k; }
    }
    for (int64_t k = 0; k < na; ++k) {
        const double dx = aortic[3 * k] - ref[0], dy = aortic[3 * k + 1] - ref[1], dz = aortic[3 * k + 2] - ref[2];
        const double d = dx * dx + dy * dy + dz * dz;
        if (d < ba) { ba = d; ka = k; }
    }
    const double vx = ref[0] - cl[kc].x, vy = ref[1] - cl[kc].y, vz = ref[2] - cl[kc].z;             // :52
    const double nn = std::sqrt(vx * vx + vy * vy + vz * vz);
    if (!(nn > 0.0)) return MM_OK;                                                                   // :53-55
    const double ux = vx / nn, uy = vy / nn, uz = vz / nn;
    const double tx = ref[0] - aortic[3 * ka], ty = ref[1] - aortic[3 * ka + 1], tz = ref[2] - aortic[3 * ka + 2];  // :59
    const double t = tx * ux + ty * uy + tz * uz;                                                    // :60
    *out = t > 0.0 ? t : 0.0;                                                                        // :62
    return MM_OK;
}

int mm_clean_outlier_points(mm_engine* h, const double* cleanup, int64_t nc, const double* reference, int64_t nr,
                            double neighborhood_radius, double min_neighbor_ratio, uint8_t* to_reference)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (nc < 0 || nr < 0 || (nc > 0 && (!cleanup || !to_reference)) || (nr > 0 && !reference))
        return set_error(MM_ERR_INVALID, "mm_clean_outlier_points: bad arguments");
    std::vector<uint8_t> f;
    if ((rc = clean_up_points(e, cleanup, nc, reference, nr, neighborhood_radius, min_neighbor_ratio, f))) return rc;
    if (nc > 0) std::memcpy(to_reference, f.data(), (size_t)nc);
    return MM_OK;
}

// find_points_by_cl_region_rs (:263-312)
int mm_find_points_by_cl_region(mm_engine* h, const mm_clpoint* cl, const uint32_t* cl_frame_index, int64_t ncl,
                                const double* frame_centroids, int64_t n_frames, const double* pts, int64_t n,
                                uint8_t* label)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    // (no frame at all: the reference's `frames.len() - 1` underflows and panics.  ONE frame is not an error there: the
    // mean spacing is 0.0 / 0 = NaN, no centerline point is "in range" of it, every point is proximal or distal)
    if (n < 0 || ncl <= 0 || !cl || n_frames < 1 || !frame_centroids || (n > 0 && (!pts || !label)))
        return set_error(MM_ERR_INVALID, "mm_find_points_by_cl_region: bad arguments (needs a centerline and >= 1 frame)");
    double mean_dz = 0.0;                                                              // :268-272
    for (int64_t i = 1; i < n_frames; ++i) mean_dz += std::fabs(frame_centroids[3 * i + 2] - frame_centroids[3 * (i - 1) + 2]);
    mean_dz /= (double)(n_frames - 1);
    // find_cl_points_in_range (:314-338): frame indices of the centerline points within mean_dz of a frame centroid
    auto fidx = [&](int64_t k) { return cl_frame_index ? cl_frame_index[k] : (uint32_t)k; };
    std::vector<uint32_t> in_range;
    const double rr = mean_dz * mean_dz;
    for (int64_t f = 0; f < n_frames; ++f)
        for (int64_t k = 0; k < ncl; ++k) {
            const double dx = frame_centroids[3 * f] - cl[k].x, dy = frame_centroids[3 * f + 1] - cl[k].y,
                         dz = frame_centroids[3 * f + 2] - cl[k].z;
            if (dx * dx + dy * dy + dz * dz <= rr) in_range.push_back(fidx(k));
        }
    std::sort(in_range.begin(), in_range.end());
    in_range.erase(std::unique(in_range.begin(), in_range.end()), in_range.end());
    const double* dref = frame_centroids + 3 * (n_frames - 1);                        // :279
    // first pass (:289-300): between = the closest centerline point (first minimum, :245-260) is one of those;
    // second pass (:303-309): the rest is proximal if it exceeds the last centroid in all three coordinates
    std::vector<uint8_t> cls((size_t)n, 0);   // 0 proximal, 1 distal, 2 between
    constexpr int64_t kBlock = 256;
    parallel_for((int)((n + kBlock - 1) / kBlock), [&](int blk) {
        const int64_t i0 = (int64_t)blk * kBlock;
        for (int64_t i = i0; i < std::min(n, i0 + kBlock); ++i) {
            const double x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
            double best = DBL_MAX;
            int64_t kb = 0;
            for (int64_t k = 0; k < ncl; ++k) {
                const double dx = x - cl[k].x, dy = y - cl[k].y, dz = z - cl[k].z;
                const double d = dx * dx + dy * dy + dz * dz;
                if (d < best) { best = d; kb = k; }
            }
            if (std::binary_search(in_range.begin(), in_range.end(), fidx(kb))) cls[(size_t)i] = 2;
            else cls[(size_t)i] = (x > dref[0] && y > dref[1] && z > dref[2]) ? 0 : 1;
        }
    });
    std::vector<double> prox, dist, betw;
    std::vector<int64_t> iprox, idist;
    for (int64_t i = 0; i < n; ++i) {
        std::vector<double>& dst = cls[(size_t)i] == 0 ? prox : (cls[(size_t)i] == 1 ? dist : betw);
        dst.insert(dst.end(), pts + 3 * i, pts + 3 * i + 3);
        if (cls[(size_t)i] == 0) iprox.push_back(i); else if (cls[(size_t)i] == 1) idist.push_back(i);
        label[i] = cls[(size_t)i];
    }
    // :310-313 the two clean-ups; the second one sees the points the first one moved into `between`
    std::vector<uint8_t> mv;
    if ((rc = clean_up_points(e, prox.data(), (int64_t)iprox.size(), betw.data(), (int64_t)(betw.size() / 3), 1.0, 0.6, mv))) return rc;
    for (size_t k = 0; k < iprox.size(); ++k)
        if (mv[k]) { label[iprox[k]] = 3; betw.insert(betw.end(), pts + 3 * iprox[k], pts + 3 * iprox[k] + 3); }
    if ((rc = clean_up_points(e, dist.data(), (int64_t)idist.size(), betw.data(), (int64_t)(betw.size() / 3), 1.0, 0.6, mv))) return rc;
    for (size_t k = 0; k < idist.size(); ++k)
        if (mv[k]) label[idist[k]] = 4;
    return MM_OK;
}


// ---- mesh labelling ---------------------------------------------------------------------------------------------

// find_centerline_bounded_points (label_coronary.rs:201-235)
int64_t mm_centerline_bounded_points(mm_engine* h, const mm_clpoint* cl, int64_t ncl, const double* pts, int64_t n,
                                     double radius, uint8_t* inside)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (n < 0 || ncl < 0 || (n > 0 && (!pts || !inside)) || (ncl > 0 && !cl))
        return set_error(MM_ERR_INVALID, "mm_centerline_bounded_points: bad arguments");
    if (n == 0 || ncl == 0) return set_error(MM_ERR_INVALID, "find_centerline_bounded_points failed because `Centerline` is empty");   // :206-209
    const std::vector<double> c = cl_xyz(cl, ncl);
    std::vector<std::vector<uint32_t>> cnt;
    if ((rc = radius_counts(e, {Set3{pts, n}, Set3{c.data(), ncl}}, {{0, 1}}, radius * radius, cnt))) return rc;   // :226
    int64_t k = 0;
    for (int64_t i = 0; i < n; ++i) { inside[i] = cnt[0][(size_t)i] > 0 ? 1 : 0; k += inside[i]; }
    return k;
}

// find_faces_near_points (:242-289)
int64_t mm_faces_near_points(mm_engine* h, const double* vertices, int64_t nv, const int64_t* faces, int64_t nf,
                             const double* pts, int64_t n, double tol, uint8_t* face_selected)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (nv < 0 || nf < 0 || n < 0 || (nv > 0 && !vertices) || (nf > 0 && (!faces || !face_selected)) || (n > 0 && !pts))
        return set_error(MM_ERR_INVALID, "mm_faces_near_points: bad arguments");
    if (nf > 0) std::memset(face_selected, 0, (size_t)nf);
    if (n == 0 || nv == 0 || nf == 0) return 0;                                                   // :248-250
    if ((rc = faces_in_range(faces, nf, nv, "mm_faces_near_points"))) return rc;
    std::vector<std::vector<uint32_t>> cnt;
    if ((rc = radius_counts(e, {Set3{vertices, nv}, Set3{pts, n}}, {{0, 1}}, tol * tol, cnt))) return rc;   // :259-273
    int64_t k = 0;
    for (int64_t f = 0; f < nf; ++f) {
        const int64_t* v = faces + 3 * f;
        face_selected[f] = (cnt[0][(size_t)v[0]] | cnt[0][(size_t)v[1]] | cnt[0][(size_t)v[2]]) ? 1 : 0;
        k += face_selected[f];
    }
    return k;
}

// remove_occluded_points_ray_triangle_rust (:70-197)
int64_t mm_occluded_points(mm_engine* h, const mm_clpoint* cl_coronary, int64_t ncc, const mm_clpoint* cl_aorta,
                           int64_t nca, double range_mm, const double* pts, int64_t n, const double* tri, int64_t nf,
                           double step_size_mm, uint8_t* removed, uint8_t* face_excluded)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (ncc < 0 || nca < 0 || n < 0 || nf < 0 || (ncc > 0 && !cl_coronary) || (nca > 0 && !cl_aorta) ||
        (n > 0 && (!pts || !removed)) || (nf > 0 && !tri))
        return set_error(MM_ERR_INVALID, "mm_occluded_points: bad arguments");
    std::vector<uint8_t> rm, ex;
    if ((rc = occluded_points(e, cl_coronary, ncc, cl_aorta, nca, range_mm, pts, n, tri, nf, step_size_mm, rm, ex))) return rc;
    int64_t k = 0;
    for (int64_t i = 0; i < n; ++i) { removed[i] = rm[(size_t)i]; k += rm[(size_t)i]; }
    if (face_excluded && nf > 0) std::memcpy(face_excluded, ex.data(), (size_t)nf);
    return k;
}

// find_aortic_points (:296-313)
int64_t mm_find_aortic_points(const double* vertices, int64_t nv, const double* a, int64_t na, const double* b,
                              int64_t nb, uint8_t* keep)
{
    if (nv < 0 || na < 0 || nb < 0 || (nv > 0 && (!vertices || !keep)) || (na > 0 && !a) || (nb > 0 && !b))
        return set_error(MM_ERR_INVALID, "mm_find_aortic_points: bad arguments");
    std::unordered_set<BitsKey, BitsHash> ex;
    ex.reserve((size_t)(na + nb));
    for (int64_t i = 0; i < na; ++i) ex.insert(bits_key(a + 3 * i));
    for (int64_t i = 0; i < nb; ++i) ex.insert(bits_key(b + 3 * i));
    int64_t k = 0;
    for (int64_t i = 0; i < nv; ++i) { keep[i] = ex.count(bits_key(vertices + 3 * i)) ? 0 : 1; k += keep[i]; }
    return k;
}

// final_reclassification (:337-640)
int mm_final_reclassification(const double* vertices, int64_t nv, const int64_t* faces, int64_t nf, const double* rca,
                              int64_t nr, const double* lca, int64_t nl, const double* rca_rm, int64_t nrr,
                              const double* lca_rm, int64_t nlr, uint8_t* label)
{
    if (nv < 0 || nf < 0 || nr < 0 || nl < 0 || nrr < 0 || nlr < 0 || (nv > 0 && (!vertices || !label)) ||
        (nf > 0 && !faces) || (nr > 0 && !rca) || (nl > 0 && !lca) || (nrr > 0 && !rca_rm) || (nlr > 0 && !lca_rm))
        return set_error(MM_ERR_INVALID, "mm_final_reclassification: bad arguments");
    if (const int rc = faces_in_range(faces, nf, nv, "mm_final_reclassification")) return rc;
    std::unordered_map<BitsKey, int64_t, BitsHash> idx;                                   // :353-358 the last index wins
    idx.reserve((size_t)nv);
    for (int64_t i = 0; i < nv; ++i) idx[bits_key(vertices + 3 * i)] = i;
    std::vector<uint8_t> labels((size_t)nv, 0);
    auto apply = [&](const double* p, int64_t m, uint8_t l) {                             // :360-383 rca, lca, rca_rm, lca_rm
        for (int64_t i = 0; i < m; ++i) {
            const auto it = idx.find(bits_key(p + 3 * i));
            if (it != idx.end()) labels[(size_t)it->second] = l;
        }
    };
    apply(rca, nr, 1); apply(lca, nl, 2); apply(rca_rm, nrr, 3); apply(lca_rm, nlr, 4);
    Adjacency adj;
    build_adjacency(faces, nf, nv, adj);
    std::vector<uint8_t> out = labels;
    reclassify_minority(adj, labels, out, 0, {1, 2});                                      // :396-398 Logic A
    reclassify_minority(adj, labels, out, 1, {0});
    reclassify_minority(adj, labels, out, 2, {0});
    restore_removed(adj, labels, out, 3, 1);                                               // :412-413 Logic B
    restore_removed(adj, labels, out, 4, 2);
    if (nv > 0) std::memcpy(label, out.data(), (size_t)nv);
    return MM_OK;
}

// centerline_based_diameter_morphing (scale_coronary.rs:218-260) on the device, n_jobs at once
int mm_centerline_morph_batch(mm_engine* h, int n_jobs, const mm_clpoint* cl, const int64_t* cl_off,
                              const double* pts_xyz, const int64_t* pt_off, const double* adj, double* out_xyz,
                              int32_t* nearest)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (n_jobs < 0 || (n_jobs > 0 && (!cl_off || !pt_off || !adj)))
        return set_error(MM_ERR_INVALID, "mm_centerline_morph_batch: bad arguments");
    if (n_jobs == 0) return MM_OK;
    if (!offsets_ok(cl_off, n_jobs) || !offsets_ok(pt_off, n_jobs))
        return set_error(MM_ERR_INVALID, "mm_centerline_morph_batch: offsets must start at 0 and not decrease");
    if ((pt_off[n_jobs] > 0 && (!pts_xyz || !out_xyz || !nearest)) || (cl_off[n_jobs] > 0 && !cl))
        return set_error(MM_ERR_INVALID, "mm_centerline_morph_batch: bad arguments");
    for (int j = 0; j < n_jobs; ++j)
        if (pt_off[j + 1] > pt_off[j] && cl_off[j + 1] == cl_off[j])                       // centerline.points[0] panics
            return set_error(MM_ERR_INVALID, "mm_centerline_morph_batch: a job with points has an empty centerline");
    return cl_morph(e, n_jobs, cl, cl_off, pts_xyz, pt_off, adj, out_xyz, nearest);
}

// the reference's coord_to_idx lookups (bits_key): the last key of each bit pattern
int64_t mm_match_points(const double* keys, int64_t nk, const double* queries, int64_t nq, int64_t* index)
{
    if (nk < 0 || nq < 0 || (nk > 0 && !keys) || (nq > 0 && (!queries || !index)))
        return set_error(MM_ERR_INVALID, "mm_match_points: bad arguments");
    std::unordered_map<BitsKey, int64_t, BitsHash> idx;
    idx.reserve((size_t)nk);
    for (int64_t i = 0; i < nk; ++i) idx[bits_key(keys + 3 * i)] = i;
    int64_t k = 0;
    for (int64_t i = 0; i < nq; ++i) {
        const auto it = idx.find(bits_key(queries + 3 * i));
        index[i] = it == idx.end() ? -1 : it->second;
        k += index[i] >= 0;
    }
    return k;
}

// keep_largest_connected_component (ccta_py.rs:541-580)
int64_t mm_keep_largest_component(const double* vertices, int64_t nv, const int64_t* faces, int64_t nf,
                                  const double* pts, int64_t n, int64_t* keep)
{
    if (nv < 0 || nf < 0 || n < 0 || (nv > 0 && !vertices) || (nf > 0 && !faces) || (n > 0 && (!pts || !keep)))
        return set_error(MM_ERR_INVALID, "mm_keep_largest_component: bad arguments");
    for (int64_t k = 0; k < 3 * nf; ++k)
        if (faces[k] < 0) return set_error(MM_ERR_INVALID, "mm_keep_largest_component: negative face index");
    if (n < 2) return 0;                                                                   // :548-550
    std::unordered_map<BitsKey, int64_t, BitsHash> idx;                                   // :552-555 the last index wins
    idx.reserve((size_t)nv);
    for (int64_t i = 0; i < nv; ++i) idx[bits_key(vertices + 3 * i)] = i;
    std::vector<uint8_t> in((size_t)nv, 0);
    bool any = false;
    for (int64_t i = 0; i < n; ++i) {                                                      // :557-561
        const auto it = idx.find(bits_key(pts + 3 * i));
        if (it != idx.end()) { in[(size_t)it->second] = 1; any = true; }
    }
    if (!any) return 0;                                                                    // :562-564
    Adjacency adj;
    build_adjacency(faces, nf, nv, adj);
    std::vector<int64_t> comp;
    std::vector<std::vector<int64_t>> comps;
    components(adj, nv, [&](int64_t v) { return in[(size_t)v] != 0; }, comp, comps);
    std::vector<int64_t>& largest = comps[largest_component(comps)];                     // :567-571
    std::sort(largest.begin(), largest.end());
    std::copy(largest.begin(), largest.end(), keep);
    return (int64_t)largest.size();
}

}  // extern "C"
