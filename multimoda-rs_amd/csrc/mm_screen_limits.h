// mm_screen_limits.h -- the set sizes, tile counts and LDS budgets that the search kernels (mm_kernels.hip) and the host code
// that plans a level for them (mm_level_plan.cpp) must agree on.  Plain constexpr arithmetic and no HIP header: the planner
// compiles without one, and the kernels call the same functions.  Internal.
#pragma once

#include <stddef.h>

namespace mm {

// ---- matrix-pipe screen (k_screen_mx, k_screen_mx_cull) ----
constexpr int kMxNctMin = 2, kMxNctMax = 17;   // column tiles of one block (the generated asm's MM_SCREEN_MX_NCT_MIN / _MAX)
constexpr int kMxRedStride = 144;              // bytes a lane of one wave's reduction scratch (MM_SCREEN_MX_RED_STRIDE)
constexpr int kMxRowTilesMax = 64;             // row tiles (LDS: 1 KB of fragments per row tile)
constexpr int kMxItemMax = 64;                 // candidates of one work item, at most (the engine's apb)
constexpr int kMxMinPoints = 64;               // smaller sets take no f32 screen
constexpr int kMxCullRowTilesMax = 17;         // the culled screen's row tiles
// Column tiles from which the culled screen loops over the set mask bits; below it keeps the bit-test chain and one tile
// pair per lane.  The static budget (profiles/r6_cull_isa_budget.txt) has the loop cheaper from 9 column tiles on (a register
// vector of fewer is indexed by compare and select) and dearer below; on the device it was measured to win at 17 and to lose
// on the small launches at 16 (profiles/r6_config3_cull_kernel_stats.csv), so only 17 takes it.
constexpr int kMxCullSetbitMinNct = 17;

constexpr int mx_min_points() { return kMxMinPoints; }
constexpr int mx_max_points() { return kMxRowTilesMax * 32; }

// the variant for a target set of nb points: column tiles per block, and whether the set takes several blocks
inline void mx_variant(int nb, int* nct, int* multi)
{
    const int nbt = (nb + 31) / 32;
    if (nbt <= kMxNctMax) { *nct = nbt < kMxNctMin ? kMxNctMin : nbt; *multi = 0; return; }
    const int nblk = (nbt + kMxNctMax - 1) / kMxNctMax;
    *nct = (nbt + nblk - 1) / nblk; *multi = 1;
}

// the culled screen takes the launch groups of this variant and row-tile cap
constexpr bool mx_cull_takes(int nct, int multi, int a_cap)
{
    return !multi && nct >= kMxNctMin && nct <= kMxNctMax && a_cap >= 1 && a_cap <= kMxCullRowTilesMax;
}

// candidates per group (WorkItem::pad) the culled screen of nct column tiles takes
constexpr int mx_cull_group_max(int nct) { return nct >= kMxCullSetbitMinNct && nct <= kMxNctMax ? 8 : 1; }

constexpr size_t lds_bytes_mx(int nct, bool multi, int a_cap, int waves)
{
    return (size_t)a_cap * 64 * 16 + (size_t)waves * nct * 64 * 8 + (size_t)waves * (32 * (kMxRedStride / 4)) * 4 +
           (multi ? (size_t)waves * a_cap * 32 * 4 : 0) + (size_t)kMxItemMax * 12;
}

// (row fragments, the waves' column fragments, per wave a row store and the thr table, the circles, the item's candidates, and
// at the end, where the set-bit variant pairs its followers, per wave the row store of a pair's second follower)
constexpr size_t lds_bytes_mx_cull(int nct, int a_cap)
{
    return (size_t)a_cap * 64 * 16 + (size_t)4 * nct * 64 * 8 + (size_t)4 * a_cap * 32 * 4 * 2 + (size_t)(nct + a_cap) * 16 +
           (size_t)kMxItemMax * 12 + (nct >= kMxCullSetbitMinNct ? (size_t)4 * a_cap * 32 * 4 : 0);
}
static_assert(2 * lds_bytes_mx_cull(kMxNctMax, kMxCullRowTilesMax) <= 160 * 1024,
              "k_screen_mx_cull: two workgroups a CU at the largest row and column tile counts");

// ---- direct-form, packed-FMA and exact kernels: the target set in LDS ----
constexpr int LDS_CAP = 160 * 1024 - 256;

constexpr size_t lds_bytes_f32(int nbp) { return (size_t)nbp * (8 + 8 + 4) + 16; }
constexpr size_t lds_bytes_f64(int nbp) { return (size_t)nbp * (16 + 16 + 8) + 16; }
constexpr size_t lds_bytes_fast(int nbp) { return (size_t)nbp * (16 + 8 + 4) + 16; }
constexpr int max_target_points_f32() { return ((LDS_CAP - 16) / 20) & ~15; }
constexpr int max_target_points_f64() { return ((LDS_CAP - 16) / 40) & ~15; }
constexpr int max_target_points_fast() { return ((LDS_CAP - 16) / 28) & ~15; }
constexpr int max_rows_fast() { return 16 * 33; }   // the packed-FMA kernel keeps one row block in registers

// ---- bounded screen ----
constexpr int kLbRowPairs = 5;      // row PAIRS per row group: query sets up to 8 * kLbRowPairs points
constexpr int kLbCandidateStep = 8; // first round: every 8th candidate (and the last) gets a bound
constexpr int kLbListQueries = 8;   // decisive points per side that the third round takes as queries

constexpr int lb_max_query_points() { return 8 * kLbRowPairs; }   // subset size the bound kernel holds in registers
constexpr int lb_max_points() { return 4096; }                    // largest set (either side) the bound kernel stages in LDS
constexpr int lb_mx_max_points() { return 1024; }                 // ... the matrix-pipe bound kernel: 32 row tiles per set, 64 KB of row fragments
constexpr size_t lds_bytes_lb(int nap, int nbp) { return ((size_t)nap + (size_t)nbp) * 16; }
constexpr int lb_candidate_step() { return kLbCandidateStep; }
// number of candidates the sparse first round scores for a list of n: 0, 8, 16, ... and n - 1
constexpr int lb_sparse_candidates(int n) { return n <= 0 ? 0 : (n - 1 + kLbCandidateStep - 1) / kLbCandidateStep + 1; }
constexpr int lb_list_queries() { return kLbListQueries; }

}  // namespace mm
