// The level planner (csrc/mm_level_plan.cpp) as a program of its own: compiled without a HIP header in sight -- that it
// builds is the proof that planning a level needs no device -- it plans a matrix-pipe level, a bounded one, an exact one
// and an empty one, lays a heap block of exactly lvl_bytes under each layout and writes every region end to end with a
// byte value of its own.  The regions must be disjoint, stay inside the block, be aligned for their element type, keep
// distinct offsets where they are empty, and the input regions must end at lvl_in_bytes; a sanitizer build sees any
// region that leaves the block.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mm_level_plan.h"
#include "mm_screen_limits.h"

using namespace mm;

static std::string g_error;
int mm::set_error(int code, const std::string& msg) { g_error = msg; return code; }

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, g_error.c_str()); return 1; } } while (0)

struct Region { const char* name; size_t off, bytes, align; };

static int check_layout(const LevelPlan& lp)
{
    const LevelLayout& l = lp.lay;
    const size_t P = (size_t)lp.P, A = (size_t)lp.A, T = (size_t)lp.T, lb = lp.use_lb ? 1 : 0, wi = sizeof(WorkItem);
    const std::vector<Region> in = {
        {"pairs", l.pairs, P * sizeof(PairDesc), alignof(PairDesc)}, {"work", l.work, (size_t)lp.W * wi, alignof(WorkItem)},
        {"work_lb", l.work_lb, (size_t)lp.W_lb * wi, alignof(WorkItem)}, {"cos32", l.cos32, T * 4, 4}, {"sin32", l.sin32, T * 4, 4},
        {"cos64", l.cos64, T * 8, 8}, {"sin64", l.sin64, T * 8, 8}, {"ang64", l.ang64, T * 8, 8}};
    std::vector<Region> all = in;
    const std::vector<Region> rest = {
        {"sq32", l.sq32, A * 4, 4}, {"sq64", l.sq64, A * 8, 8}, {"flag", l.flag, A, 1}, {"items", l.items, A * wi, alignof(WorkItem)},
        {"n_items", l.n_items, 32, 4}, {"lb32", l.lb32, lb * A * 4, 4}, {"pick", l.pick, lb * P * 8, 4},
        {"items_pick", l.items_pick, lb * P * 2 * wi, alignof(WorkItem)},
        {"items_lb", l.items_lb, lb * (size_t)lp.lb_runs_cap * 3 * wi, alignof(WorkItem)},
        {"klist", l.klist, lp.kept_nct > 0 ? A * 4 : 0, 4}, {"emit", l.emit, lb * P * (size_t)(l.emit_rows + l.emit_cols) * 4, 4},
        {"qlist", l.qlist, lb * P * 2 * (size_t)lb_list_queries() * 4, 4}, {"best_cost", l.best_cost, P * 8, 8},
        {"best_idx", l.best_idx, P * 4, 4}, {"n_rescored", l.n_rescored, P * 4, 4}, {"near_cnt", l.near_cnt, P * 4, 4},
        {"near_idx", l.near_idx, P * 4 * kMaxNear, 4}};
    all.insert(all.end(), rest.begin(), rest.end());
    if (lp.want_costs) all.push_back({"all_costs", l.off_all_costs, A * 8, 8});
    else CHECK(l.off_all_costs == 0);
    CHECK(l.lvl_bytes > 0 && l.lvl_bytes % 256 == 0 && l.lvl_in_bytes % 256 == 0);
    CHECK(l.emit_rows >= lp.max_na && l.emit_cols >= lp.max_nt && l.emit_rows % 4 == 0 && l.emit_cols % 4 == 0);
    unsigned char* block = (unsigned char*)std::aligned_alloc(256, l.lvl_bytes);   // hipMalloc's alignment at the least
    CHECK(block);
    for (size_t k = 0; k < all.size(); ++k) {
        const Region& r = all[k];
        CHECK(r.off + r.bytes <= l.lvl_bytes);
        CHECK(r.off % 256 == 0 && (size_t)(block + r.off) % r.align == 0);
        if (k) CHECK(r.off > all[k - 1].off && r.off >= all[k - 1].off + all[k - 1].bytes);   // in order, an offset each
        std::memset(block + r.off, (int)(k + 1), r.bytes);
    }
    for (size_t k = 0; k < all.size(); ++k)
        for (size_t i = 0; i < all[k].bytes; ++i)
            if (block[all[k].off + i] != (unsigned char)(k + 1)) { std::printf("region %s overwritten\n", all[k].name); return 1; }
    std::free(block);
    // one upload of the inputs, one copy back of the results
    for (const Region& r : in) CHECK(r.off + r.bytes <= l.lvl_in_bytes);
    CHECK(l.sq32 == l.lvl_in_bytes);
    CHECK(l.off_best_cost == l.best_cost && l.near_idx + P * 4 * kMaxNear <= l.off_best_cost + l.res_bytes);
    CHECK(l.off_best_cost + l.res_bytes <= l.lvl_bytes);
    CHECK(l.r_best_idx == l.best_idx - l.best_cost && l.r_n_rescored == l.n_rescored - l.best_cost);
    CHECK(l.r_near_cnt == l.near_cnt - l.best_cost && l.r_near_idx == l.near_idx - l.best_cost);
    return 0;
}

struct Sets {
    std::vector<int32_t> off, len, main; std::vector<double> rho;
    void add(int n, double r, int m = 0) { off.push_back(off.empty() ? 0 : off.back() + len.back()); len.push_back(n); rho.push_back(r); main.push_back(m); }
};

static int plan(const Sets& s, const std::vector<PairSpec>& pairs, int precision, bool want_costs, const ScreenOptions& opts, LevelPlan& lp)
{
    return plan_level(s.off, s.len, s.rho, s.main, pairs, precision, 0, INT32_MAX, want_costs, opts, lp);
}

int main()
{
    std::vector<double> angles(361);
    for (size_t i = 0; i < angles.size(); ++i) angles[i] = (double)i * 0.5 * M_PI / 180.0;
    Sets s;
    s.add(544, 3.1); s.add(300, 3.0, 192); s.add(65, 2.9); s.add(0, 0.0); s.add(257, 3.2);
    auto pair = [&](int a, int b) { return PairSpec{a, b, 0.0, 0.0, 0, angles.data(), (int32_t)angles.size(), 0.0, 0.0}; };
    ScreenOptions opts;
    LevelPlan lp;   // one plan, planned again and again: the vectors are refilled in place

    // matrix pipe: culled groups of three shapes, a split set, a pair without candidates to launch
    CHECK(plan(s, {pair(0, 0), pair(1, 0), pair(2, 1), pair(1, 3), pair(4, 4)}, MM_PRECISION_F32_MATRIX, true, opts, lp) == MM_OK);
    CHECK(lp.precision == MM_PRECISION_F32_MATRIX && lp.P == 5 && lp.A == 4 * 361 && lp.trivial[3] == 1);
    CHECK(lp.T == 361 + 1 + 361);   // the empty-set pair keeps one entry and ends the run of pairs that share the first table
    CHECK(lp.groups.size() == 3 && lp.groups[0].screen == Screen::MatrixCull && lp.host_pairs[1].ref_main == 192);
    CHECK(lp.W == (int)lp.host_work.size() && lp.W_lb == 0 && lp.lay.off_all_costs > 0);
    if (check_layout(lp)) return 1;

    // bounded search on the matrix pipe, then on the packed-FMA kernels
    opts.bound_min_candidates = 0;
    CHECK(plan(s, {pair(1, 1), pair(1, 1)}, MM_PRECISION_F32_BOUNDED, false, opts, lp) == MM_OK);
    CHECK(lp.use_lb && lp.kept_nct == 10 && lp.W_lb == (int)lp.host_work_lb.size() && lp.W_lb > 0 && lp.groups.empty());
    if (check_layout(lp)) return 1;
    opts.bound_matrix = false;
    CHECK(plan(s, {pair(1, 1), pair(1, 4)}, MM_PRECISION_F32_BOUNDED, false, opts, lp) == MM_OK);
    CHECK(lp.use_lb && lp.kept_nct == 0 && lp.lb_stride >= 8);
    if (check_layout(lp)) return 1;

    // exact, and an f32 level that a set no f32 screen can hold turns exact
    CHECK(plan(s, {pair(0, 1), pair(2, 3)}, MM_PRECISION_F64, true, opts, lp) == MM_OK);
    CHECK(lp.precision == MM_PRECISION_F64 && lp.groups.empty() && !lp.use_lb && lp.host_work_lb.empty());
    if (check_layout(lp)) return 1;
    Sets big = s;
    big.rho[0] = INFINITY;
    CHECK(plan(big, {pair(0, 1)}, MM_PRECISION_F32_MATRIX, false, opts, lp) == MM_OK && lp.precision == MM_PRECISION_F64);
    if (check_layout(lp)) return 1;

    // empty: no pairs at all, and pairs whose slice of the candidate axis is empty
    CHECK(plan(s, {}, MM_PRECISION_F32_MATRIX, false, opts, lp) == MM_OK);
    CHECK(lp.P == 0 && lp.W == 0 && lp.A == 0 && lp.T == 0 && lp.host_work.empty() && lp.groups.empty());
    if (check_layout(lp)) return 1;
    CHECK(plan_level(s.off, s.len, s.rho, s.main, {pair(0, 1)}, MM_PRECISION_F32_MATRIX, 400, 500, false, opts, lp) == MM_OK);
    CHECK(lp.P == 1 && lp.A == 0 && lp.W == 0);
    if (check_layout(lp)) return 1;

    // errors come back through set_error with the engine's messages
    CHECK(plan(s, {pair(0, 7)}, MM_PRECISION_F32, false, opts, lp) == MM_ERR_INVALID && g_error == "pair references a set that was not staged");
    CHECK(plan(s, {pair(0, 1)}, 17, false, opts, lp) == MM_ERR_INVALID);
    std::printf("level_plan_host OK\n");
    return 0;
}
