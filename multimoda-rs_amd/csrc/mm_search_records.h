// mm_search_records.h -- the search engine's records, shared by the kernels (mm_kernels.hip), the host code that stages them
// (mm_engine.cpp) and the level planner (mm_level_plan.cpp).  No HIP header: the planner compiles without one.  Internal.
#pragma once

#include <stdint.h>

namespace mm {

// One (reference set, target set, candidate list) search.  Point sets live in one pool
// (several pairs may share a set: frame i is the target of pair i and the reference of
// pair i+1); cos/sin tables are shared between pairs with identical candidate lists.
struct PairDesc {
    int32_t ref_off, n_ref;   // into the point pool
    int32_t tgt_off, n_tgt;
    int32_t tab_off;          // into the cos/sin tables
    int32_t out_off;          // into the per-candidate outputs
    int32_t n_ang;            // candidates of this pair in this plan (slice)
    int32_t flags;            // MM_SEARCH_SKIP_ZERO
    int32_t ang_full;         // length of the pair's full candidate list (>= n_ang)
    int32_t ang_begin;        // first candidate of the slice this plan owns
    int32_t n_slice;          // candidates in the slice (== n_ang, except for empty-set pairs: n_ang = 0 there)
    int32_t pad0;             // k_screen_mx: scale exponent e (coordinates are multiplied by 2^e); otherwise 0
    int32_t ref_main, tgt_main;   // k_screen_mx_cull: > 0 -- the set is two runs (main points, then the rest) and each run
                                  // starts a tile of its own (mm_tile_slot_point, mm_tile_bound.h); 0: the points in order
    double  cx, cy;           // rotation centre (exact kernel)
    double  delta;            // f32 screening error bound (same unit as the costs)
    double  tol2;             // candidates within tol2 of the exact minimum are reported as near-ties
    double  e2;               // absolute error bound of the screened SQUARED value (fast kernel; else 0)
    double  rho_t;            // largest distance of a target point from the rotation centre
};

// Source of one search set of the within-pullback search, built on the device from the raw pullback
// (align_within.rs:173-191: downsample(lumen, S) ++ downsample(catheter, ceil(n_cath * S / len_lumen0)),
// contour.rs:47-58), centred on the frame's centroid.  Raw pool = xyz triples (f64) as the caller holds them.
struct SetSrc {
    int64_t lum_at;           // first lumen point of the frame in the raw pool (point index)
    int64_t cath_at;          // first catheter point of the frame (unused when cath_take == 0)
    int32_t lum_len, lum_take;    // points of the contour, points asked for
    int32_t cath_len, cath_take;
    int32_t dst_off, n;       // into the point pool; n = min(lum_len, lum_take) + min(cath_len, cath_take)
    double  cx, cy;           // the frame's centroid
};

// One workgroup's share: `cnt` consecutive candidates of one pair.
struct WorkItem {
    int32_t pair, a0, cnt, pad;   // pad: the bound kernels' candidate step; k_screen_mx_cull: candidates per group (0: 1)
};

// k_screen_mx_cull: one workgroup's RUN of work items -- `count` consecutive items of one pair, the first at `first` of its
// launch group's items (the planner's run table, mm_level_plan.h): the workgroup stages the pair once for all of them.
struct WorkRun {
    int32_t first, count;
};

static constexpr int kMaxNear = 8;  // near-tie slots per pair (MM_MAX_NEAR)

struct BatchDev {
    const PairDesc* pairs;
    const WorkItem* work;
    int32_t n_pairs, n_work;
    // point pool: f32 copy relative to the set's centre, f64 copy as given
    const float *p32x, *p32y;
    const double *p64x, *p64y;
    // candidate tables
    const float *cos32, *sin32;
    const double *cos64, *sin64;
    const double *ang64;      // the candidate angles themselves (same indexing): device-side exchange records
    // per-candidate outputs
    float*    sq32;       // squared Hausdorff from the screening kernel
    double*   sq64;       // exact squared Hausdorff (valid where flag != 0 or in exact mode)
    uint8_t*  flag;       // 1 = shortlisted (re-scored in f64); before that, bounded search on the matrix pipe: 1 = needs a bound
    int64_t   n_cand;     // candidates of the level (length of sq32 / lb32 / flag)
    // shortlist queue
    WorkItem* items;      // capacity = total candidates (bounded mode: first the survivors' runs)
    int32_t*  n_items;    // 8 device counters: [0] re-score queue; bounded mode: [1] picks, [2] queue 0 (round 2),
                          // [3] queue 1 (round 3), [4] second picks, [5] queue 2 (survivors)
    // bounded screen (MM_PRECISION_F32_BOUNDED)
    const WorkItem* work_lb;   // bound kernel's work list (more candidates per workgroup)
    int32_t   n_work_lb, lb_stride;
    int32_t   lb_mx;       // bounded search on the matrix pipe: row tiles per set of k_bound_mx's LDS layout
    int32_t   lb_mx_qt, lb_mx_nc;   // its variant: column tiles of queries per side (1 | 2), candidates per wave at once (1 | 2)
    int32_t   kept_mx_nct, kept_mx_acap;   // > 0: the bounded search runs on the matrix pipe; the picks' and the survivors'
                                           // screen is k_screen_mx<kept_mx_nct, false> (every pair) with LDS for kept_mx_acap row tiles
    float*    lb32;        // per-candidate lower bound of the screened squared value
    int32_t*  pick_idx;    // [2 * n_pairs] per pair: candidate with the smallest bound after round 1 / round 3 (-1: none)
    WorkItem* items_pick;  // [2 * n_pairs] queue entries of the two picks
    WorkItem* items_lb;    // three queues of `runs cap` entries: round 2, round 3, survivors
    int32_t*  klist;       // [n_cand] per pair (at its out_off): the survivors' candidate indices (k_lb_keep_mx)
    float*    emit;        // per pair emit_rows + emit_cols: row / column minima of the first pick
    int32_t   emit_rows, emit_cols;
    int32_t*  qlist;       // per pair 2 * lb_list_queries(): decisive reference / target point indices
    unsigned long long* stats;  // nullable: [1] candidates bounded in round 2, [3] in round 3, [2] fully screened
    // per-pair results
    double*   best_cost;
    int32_t*  best_idx;
    int32_t*  n_rescored;
    int32_t*  near_cnt;   // exact-scored candidates with cost <= best + tol2 (may exceed kMaxNear)
    int32_t*  near_idx;   // [n_pairs * kMaxNear] ascending candidate indices (full-list numbering)
    double*   all_costs;  // optional per-candidate sqrt'ed costs
};

}  // namespace mm
