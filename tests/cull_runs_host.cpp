// The culled screen's run table (plan_runs and Planner::form_launch_groups, csrc/mm_level_plan.cpp) as a program of its own,
// no device: it plans levels of the shapes below with ScreenOptions::screen_run automatic, off and forced, and checks on
// every culled launch group that
//   * every work item of the group is in exactly one run, in list order (the runs tile [0, work_count) without a gap);
//   * no run holds items of two pairs, and none leaves its launch group;
//   * a forced size is honoured up to the pair's items: a run is shorter only where the pair ends;
//   * the automatic sizes never grow along the list but behind a run that its pair's end cut short, the largest is
//     work_count / (16 x 512), the launch keeps 16 rounds of 512 workgroups, and the list ends in single items;
//   * a launch below the limit, a launch with the switch off and every launch of another screen has no run table, and a
//     level without a table has no `runs` region: its layout is the one planned with the switch off.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "mm_level_plan.h"
#include "mm_screen_limits.h"

using namespace mm;

static std::string g_error;
int mm::set_error(int code, const std::string& msg) { g_error = msg; return code; }

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s (%s)\n", __FILE__, __LINE__, #c, g_error.c_str()); return 1; } } while (0)

struct Sets {
    std::vector<int32_t> off, len, main; std::vector<double> rho;
    void add(int n, double r, int m = 0) { off.push_back(off.empty() ? 0 : off.back() + len.back()); len.push_back(n); rho.push_back(r); main.push_back(m); }
};

static int plan(const Sets& s, const std::vector<PairSpec>& pairs, int run, LevelPlan& lp)
{
    ScreenOptions opts;
    opts.screen_run = run;
    return plan_level(s.off, s.len, s.rho, s.main, pairs, MM_PRECISION_F32_MATRIX, 0, INT32_MAX, false, opts, lp);
}

// items of the pair that item i of the group belongs to, from i to the pair's end
static int left_of_pair(const WorkItem* w, int n, int i)
{
    int e = i + 1;
    while (e < n && w[e].pair == w[i].pair) ++e;
    return e - i;
}

// The properties of every culled group's runs for the switch `run`; *tables: the groups that have a table.
static int check_runs(const LevelPlan& lp, int run, int* tables)
{
    *tables = 0;
    size_t at = 0;
    for (const ScreenGroup& g : lp.groups) {
        if (g.screen != Screen::MatrixCull) { CHECK(g.run_count == 0); continue; }
        const WorkItem* w = lp.host_work.data() + g.work_begin;
        const int n = g.work_count;
        const int cap = run ? run : n / (kRunMinRounds * kRunResidentWgs);
        if (run == 1 || cap < 2) { CHECK(g.run_count == 0); continue; }
        ++*tables;
        CHECK(g.run_count > 0 && (size_t)g.run_begin == at && at + (size_t)g.run_count <= lp.host_runs.size());
        const WorkRun* r = lp.host_runs.data() + g.run_begin;
        at += (size_t)g.run_count;
        int next = 0, prev = INT32_MAX;
        bool prev_cut = false;
        for (int k = 0; k < g.run_count; ++k) {
            CHECK(r[k].first == next && r[k].count >= 1 && r[k].first + r[k].count <= n);      // in order, no gap, inside the group
            for (int i = 1; i < r[k].count; ++i) CHECK(w[r[k].first + i].pair == w[r[k].first].pair);
            const int left = left_of_pair(w, n, r[k].first);
            CHECK(r[k].count <= left && r[k].count <= cap);
            const bool cut = r[k].count == left;                                              // the pair ends with this run
            // the size asked for: the forced one, or the guided share of what is left of the launch; less only at a pair's end
            const int want = run ? cap : std::min(cap, std::max(1, (n - next + 2 * kRunResidentWgs - 1) / (2 * kRunResidentWgs)));
            CHECK(r[k].count == want || (cut && r[k].count < want));
            CHECK(r[k].count <= prev || prev_cut);
            prev = r[k].count;
            prev_cut = r[k].count < want;
            next += r[k].count;
        }
        CHECK(next == n);
        if (!run) {
            CHECK(g.run_count >= kRunMinRounds * kRunResidentWgs);
            for (int k = g.run_count - kRunResidentWgs; k < g.run_count; ++k) CHECK(r[k].count == 1);   // the last round: single items
            CHECK(r[0].count == std::min(cap, left_of_pair(w, n, 0)));
        }
    }
    CHECK(at == lp.host_runs.size());
    // the region: behind the other inputs and inside the one upload, or none at all
    const LevelLayout& l = lp.lay;
    if (lp.host_runs.empty()) CHECK(l.runs == 0);
    else {
        CHECK(l.runs % 256 == 0 && l.runs >= l.ang64 + (size_t)lp.T * 8 && l.runs > l.ang64);
        CHECK(l.runs + lp.host_runs.size() * sizeof(WorkRun) <= l.lvl_in_bytes && l.sq32 == l.lvl_in_bytes);
    }
    return 0;
}

// Every size of the switch on one level: the work list and the launch groups never depend on it; `auto_tables`: the groups
// that the automatic rule gives a table.
static int check_level(const char* name, const Sets& s, const std::vector<PairSpec>& pairs, int auto_tables, int want_items)
{
    LevelPlan off, lp;
    CHECK(plan(s, pairs, 1, off) == MM_OK);
    CHECK(off.host_runs.empty() && off.lay.runs == 0);
    if (want_items >= 0) CHECK(off.W == want_items);
    int culled = 0;
    for (const ScreenGroup& g : off.groups) culled += g.screen == Screen::MatrixCull;
    for (int run : {0, 2, 3, 5, 23, 64}) {
        CHECK(plan(s, pairs, run, lp) == MM_OK);
        CHECK(lp.W == off.W && lp.groups.size() == off.groups.size());
        for (int k = 0; k < lp.W; ++k) {
            const WorkItem &a = lp.host_work[(size_t)k], &b = off.host_work[(size_t)k];
            CHECK(a.pair == b.pair && a.a0 == b.a0 && a.cnt == b.cnt && a.pad == b.pad);
        }
        for (size_t k = 0; k < lp.groups.size(); ++k)
            CHECK(lp.groups[k].work_begin == off.groups[k].work_begin && lp.groups[k].work_count == off.groups[k].work_count &&
                  lp.groups[k].screen == off.groups[k].screen);
        int tables = 0;
        if (check_runs(lp, run, &tables)) { std::printf("  (%s, screen_run %d)\n", name, run); return 1; }
        CHECK(tables == (run ? culled : auto_tables));
        if (tables == 0) CHECK(lp.lay.lvl_in_bytes == off.lay.lvl_in_bytes && lp.lay.lvl_bytes == off.lay.lvl_bytes && lp.lay.sq32 == off.lay.sq32);
    }
    std::printf("%s: %d items, %d culled launch groups, %d with automatic runs\n", name, off.W, culled, auto_tables);
    return 0;
}

int main()
{
    auto list = [](int n) { std::vector<double> a((size_t)n); for (int i = 0; i < n; ++i) a[(size_t)i] = (-180.0 + 0.5 * i) * M_PI / 180.0; return a; };
    const std::vector<double> a721 = list(721), a40 = list(40), a20 = list(20);
    Sets s;
    s.add(521, 3.1, 501); s.add(521, 3.0, 501); s.add(300, 2.9);
    auto pair = [&](int a, int b, const std::vector<double>& ang) { return PairSpec{a, b, 0.0, 0.0, 0, ang.data(), (int32_t)ang.size(), 0.0, 0.0}; };

    // the flagship's shape: 4 x 511 frame pairs, 721 rotations, 23 items of 31 or 32 candidates a pair
    std::vector<PairSpec> pairs(4 * 511, pair(0, 1, a721));
    if (check_level("4 x 511 pairs x 23 items", s, pairs, 1, 4 * 511 * 23)) return 1;
    {
        LevelPlan lp;
        CHECK(plan(s, pairs, 0, lp) == MM_OK && lp.groups.size() == 1);
        const WorkRun* r = lp.host_runs.data();
        CHECK(r[0].count == 5 && r[1].count == 5 && r[2].count == 5 && r[3].count == 5 && r[4].count == 3 && r[5].first == 23);
    }

    // one pair: 181 items of 4 candidates; a forced run longer than the pair is the whole pair
    pairs.assign(1, pair(0, 1, a721));
    if (check_level("one pair", s, pairs, 0, -1)) return 1;
    {
        LevelPlan lp;
        CHECK(plan(s, pairs, 64, lp) == MM_OK && lp.groups.size() == 1 && lp.W > 64);
        CHECK(lp.host_runs.size() == (size_t)(lp.W + 63) / 64 && lp.host_runs.back().first + lp.host_runs.back().count == lp.W);
        CHECK(plan(s, pairs, 100000, lp) == MM_OK && lp.host_runs.size() == 1 && lp.host_runs[0].first == 0 && lp.host_runs[0].count == lp.W);
    }

    // below the limit: fewer than 16 rounds, and 16 rounds but not twice as many (a run of two would leave fewer than 16)
    pairs.assign(300, pair(0, 1, a721));
    if (check_level("300 pairs (13 rounds)", s, pairs, 0, 300 * 23)) return 1;
    pairs.assign(511, pair(0, 1, a721));
    if (check_level("511 pairs (22 rounds)", s, pairs, 0, 511 * 23)) return 1;

    // pairs of 23, 2 and 1 items mixed in one launch
    pairs.clear();
    for (int k = 0; k < 800; ++k) { pairs.push_back(pair(0, 1, a721)); pairs.push_back(pair(1, 0, a40)); pairs.push_back(pair(0, 1, a20)); }
    if (check_level("pairs of 23, 2 and 1 items", s, pairs, 1, 800 * 26)) return 1;

    // two launch groups (17 and 10 column tiles): the large one has runs of its own, the small one none by the rule
    pairs.assign(4 * 511, pair(0, 1, a721));
    for (int k = 0; k < 40; ++k) pairs.push_back(pair(0, 2, a721));
    if (check_level("two launch groups", s, pairs, 1, -1)) return 1;
    {
        LevelPlan lp;
        CHECK(plan(s, pairs, 3, lp) == MM_OK && lp.groups.size() == 2);
        CHECK(lp.groups[0].run_count > 0 && lp.groups[1].run_count > 0 && lp.groups[1].run_begin == lp.groups[0].run_count);
        CHECK(lp.host_runs[(size_t)lp.groups[1].run_begin].first == 0);   // counted from the group's first item
    }

    // plan_runs itself: nothing to do, and sizes that are not sizes
    std::vector<WorkRun> out;
    const WorkItem one{0, 0, 4, 0};
    CHECK(plan_runs(&one, 1, 0, out) == 0 && plan_runs(&one, 0, 5, out) == 0 && plan_runs(&one, 1, 1, out) == 0 && plan_runs(&one, 1, -3, out) == 0);
    CHECK(out.empty() && plan_runs(&one, 1, 5, out) == 1 && out[0].first == 0 && out[0].count == 1);
    std::printf("cull_runs_host OK\n");
    return 0;
}
