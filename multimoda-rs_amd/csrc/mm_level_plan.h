// mm_level_plan.h -- what a level of searches IS before anything is staged: from the sets' metadata, the pairs and the
// engine's switches, plan_level decides every pair's descriptor and screen, the work lists, the launch groups and the layout
// of the level blob.  A pure host value and no HIP header: Plan::stage_level (mm_engine.cpp) fills the tables, uploads and
// binds the device pointers from it; mm_level_plan_probe and tests/level_plan_host.cpp read it without a device.  Internal.
#pragma once

#include <climits>
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/mm_hausdorff.h"
#include "mm_search_records.h"

namespace mm {

int set_error(int code, const std::string& msg);   // mm_engine.cpp: the thread's last error (mm_last_error); returns code

// The switches that choose a level's screens.  The engine holds the defaults (mm_engine_set_*); plan_level copies
// them into the plan, and everything from there on -- the screen of every pair, the device description, run() -- reads
// the plan's copy.
struct ScreenOptions {
    int64_t bound_min_candidates = 16384;   // MM_PRECISION_F32_BOUNDED: smaller batches skip the bound rounds
    bool bound_matrix = true;               // MM_PRECISION_F32_BOUNDED: bounds, picks and survivors on the matrix pipe
    int bound_matrix_qt = 1, bound_matrix_nc = 1;   // k_bound_mx's variant: query tiles per side, candidates per wave
    bool screen_cull = true;                // MM_PRECISION_F32_MATRIX: sets of 64 .. 544 points through k_screen_mx_cull
    bool screen_split = true;               // k_screen_mx_cull: a set of two runs (lumen ++ catheter) gives each run tiles of its
                                            // own where that adds no tile (PairDesc::ref_main / tgt_main)
    int screen_group = 0;                   // k_screen_mx_cull: consecutive candidates that share one tile bound and mask set
                                            // (WorkItem::pad).  0: chosen per pair from its list (mm_tile_group_auto), never
                                            // more than a quarter of a work item; 1: off; 2 | 4 | 8: forced
    bool screen_pair = true;                // k_screen_mx_cull: a group's followers run their phase 1 two at a time (one tile
                                            // loop for both).  A launch argument: the plan is the same either way
    bool screen_floor = true;               // k_screen_mx_cull (set-bit variant): the value floor -- phase 2 only for rows and
                                            // columns whose phase-1 minimum lies above the largest minimum that is already
                                            // exact.  A launch argument too: same plan, same values, fewer tiles
    int screen_run = 0;                     // k_screen_mx_cull: consecutive work items of one pair that one workgroup runs,
                                            // staging the pair once (LevelPlan::host_runs).  0: chosen per launch group
                                            // (plan_runs: none below kRunMinRounds rounds of workgroups); 1: off, a
                                            // workgroup per item; n > 1: forced, up to the pair's items
};

// The run rule's constants (plan_runs): the workgroups of k_screen_mx_cull a device holds at once (256 CUs, two each), and
// the rounds of them a launch must keep for its end to stay even.
constexpr int kRunResidentWgs = 512;
constexpr int kRunMinRounds = 16;

struct PairSpec {          // one search
    int32_t ref_set, tgt_set;      // indices into the set list
    double cx, cy;                 // rotation centre (must equal the centre of both sets' f32 copies)
    int32_t flags;
    const double* angles; int32_t n_angles;   // candidate list (pairs passing the same pointer share tables)
    double tie_tol;                // near-tie tolerance on the exact cost (0 -> exact ties only)
    double delta_extra;            // added to the f32 screening bound
    int32_t slice_begin = 0, slice_end = INT32_MAX;   // this pair's share of the candidate axis
};

// The screen of a pair searched without bound rounds, in the order the work list lays out its groups: none (a set of fewer
// than 64 points: every candidate is scored exactly), direct-form f32, packed FMA, the matrix pipe (k_screen_mx), the
// matrix pipe without the tiles that hold no minimum (k_screen_mx_cull).
enum class Screen { None, Direct, PackedFma, Matrix, MatrixCull };

// Screens without bound rounds: the work list is grouped by screen, one launch per group, in the order of Screen and
// (multi, nct, cls).  Matrix / MatrixCull: k_screen_mx<nct, multi> / k_screen_mx_cull<nct> with LDS for a_cap row tiles;
// candidates and tiles_full (MatrixCull: the tiles the full kernel computes) feed Engine::screened / cull_tiles_full.
// MatrixCull: [run_begin, run_begin + run_count) of LevelPlan::host_runs are the group's runs; run_count == 0: none, one
// workgroup per work item.
struct ScreenGroup {
    Screen screen; int nct, multi, a_cap, work_begin, work_count;
    int64_t candidates, tiles_full;
    int run_begin = 0, run_count = 0;
};

// Byte offsets of the level blob's regions, in the order they lie: steps of 256 bytes, and an empty region still takes 16
// bytes and an offset of its own.  [pairs .. ang64] are the inputs (one upload of lvl_in_bytes), [best_cost .. near_idx] the
// result block (one copy back of res_bytes from off_best_cost; the r_* are offsets inside it), all_costs is optional.
// runs (LevelPlan::host_runs) is optional too and the last of the inputs: a level without a run table has no such region.
struct LevelLayout {
    size_t pairs = 0, work = 0, work_lb = 0, cos32 = 0, sin32 = 0, cos64 = 0, sin64 = 0, ang64 = 0, runs = 0;
    size_t sq32 = 0, sq64 = 0, flag = 0, items = 0, n_items = 0;
    size_t lb32 = 0, pick = 0, items_pick = 0, items_lb = 0, klist = 0, emit = 0, qlist = 0;
    size_t best_cost = 0, best_idx = 0, n_rescored = 0, near_cnt = 0, near_idx = 0;
    size_t lvl_in_bytes = 0, lvl_bytes = 0;
    size_t off_best_cost = 0, res_bytes = 0, off_all_costs = 0;
    size_t r_best_idx = 0, r_n_rescored = 0, r_near_cnt = 0, r_near_idx = 0;
    int emit_rows = 0, emit_cols = 0;
};

struct LevelPlan {
    int precision = MM_PRECISION_F32;         // as asked for, or MM_PRECISION_F64 where no f32 screen can hold the coordinates
    int P = 0, W = 0, W_lb = 0;               // pairs, work items, work items of the first bound round
    int64_t A = 0;                            // candidates in this plan (sum of slices)
    int64_t T = 0;                            // cos/sin table entries
    int max_na = 1, max_nbp = 16, max_nt = 1;
    bool use_fast = false;                    // expanded-form screening kernel selected
    bool use_lb = false;                      // lower-bound pass in front of the screen (MM_PRECISION_F32_BOUNDED)
    int lb_stride = 0, lb_runs_cap = 0;
    // bounded search on the matrix pipe (kept_nct > 0): row tiles of k_bound_mx's LDS layout, k_screen_mx's variant for the
    // picks and the survivors and its LDS cap (BatchDev::lb_mx, kept_mx_*)
    int lb_mx_tiles = 0, kept_nct = 0, kept_acap = 0;
    double pair_evals = 0.0;
    double lb_pair_evals = 0.0;               // pair-distances of the first bound round
    int64_t lb_sparse_total = 0;              // candidates the first bound round scores
    int32_t slice_end = INT32_MAX;
    bool want_costs = false;
    ScreenOptions opts;                       // the switches this level was planned with
    std::vector<PairDesc> host_pairs;
    std::vector<WorkItem> host_work, host_work_lb;
    std::vector<WorkRun> host_runs;           // the culled launch groups' runs (ScreenGroup::run_begin), group by group
    std::vector<double> host_tables;          // distinct candidate lists (slice-local), dev tables mirror them
    std::vector<uint8_t> trivial;             // pair has an empty set: every cost is 0.0
    std::vector<int32_t> pair_slice_end;      // per pair: end of the candidate slice this plan owns
    std::vector<ScreenGroup> groups;
    LevelLayout lay;
};

// Plan the level of `pairs` over the sets described by set_off / set_len / set_rho (largest distance of a point from the
// set's centre; inf: no f32 screen can hold the set) / set_main (> 0: the set is two runs, the first of this length), for the
// candidates [angle_begin, angle_end) of every pair's list.  `out` is refilled in place (its vectors keep their capacity).
// MM_OK, or the error set through set_error.
int plan_level(const std::vector<int32_t>& set_off, const std::vector<int32_t>& set_len, const std::vector<double>& set_rho,
               const std::vector<int32_t>& set_main, const std::vector<PairSpec>& pairs, int precision, int32_t angle_begin,
               int32_t angle_end, bool want_costs, const ScreenOptions& opts, LevelPlan& out);

// The runs of one culled launch group's work items w[0 .. n) (ScreenOptions::screen_run = run), appended to `out`: every
// item in exactly one run, in list order, and no run holds items of two pairs.  run > 1: runs of `run` items, as far as
// the pair has items.  run == 0: nothing for a launch of fewer than 2 kRunMinRounds rounds; else guided sizes -- with
// R = n / (kRunMinRounds kRunResidentWgs), the run at item i takes ceil((n - i) / (2 kRunResidentWgs)) items, at least 1
// and at most R, and never more than its pair has left: the launch keeps kRunMinRounds rounds of workgroups, the sizes
// only fall along the list (but for a run cut short by its pair's end) and the last kRunResidentWgs workgroups' worth
// of items run one by one, as without runs.  Returns the number of runs appended (0: no table, a workgroup per item).
int plan_runs(const WorkItem* w, int n, int run, std::vector<WorkRun>& out);

// The plan as 64-bit words, seven arrays each preceded by its length (doubles by bit pattern); the order is written down at
// mm_level_plan_probe (include/mm_hausdorff.h).
void serialize_level_plan(const LevelPlan& lp, std::vector<int64_t>& words);

}  // namespace mm
