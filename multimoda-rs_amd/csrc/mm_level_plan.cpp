// mm_level_plan.cpp -- plan_level: the decisions of one level of searches, step by step (mm_level_plan.h).  Host arithmetic
// only; compiled with -ffp-contract=off like the rest of the host code, and on its own by tests/level_plan_host.cpp.
#include "mm_level_plan.h"
#include "mm_screen_limits.h"
#include "mm_tile_bound.h"
#include "mm_pool.h"
#include "mm_trace.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <tuple>

namespace mm {

namespace {

inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// f32 screening error bound (DESIGN.md "screen-then-exact"): with u = 2^-24 and rho_r, rho_t
// the largest distance of a reference / target point from the rotation centre,
// |H_f32 - H_true| <= u (3.9 rho_r + 10 rho_t); we use 24 u (rho_r + rho_t).
// The screen works on coordinates relative to the rotation centre; the exact re-score is the REFERENCE's
// arithmetic on the coordinates as given, whose rotation ends with "+ cx" (contour_point.rs:45-48): its result
// is rounded at the magnitude of the coordinates, |H_f64 - H_true| <= 2^-53 (1.5 |c| + 10 rho_t + 3 rho_r).
// That term only matters for point sets a billion times smaller than their coordinates (all points of a set
// equal: every exact cost is 0.0, the screen sees 1e-17 -- found by the randomised search test), but the
// shortlist has to hold every candidate whose EXACT cost can be minimal, so it is part of the bound:
// 2^-49 (|cx| + |cy| + rho_r + rho_t), sixteen roundings at the coordinates' magnitude.
inline double screen_delta(double rho_r, double rho_t, double cx, double cy)
{
    const double u = 5.9604644775390625e-08;  // 2^-24
    return 24.0 * u * (rho_r + rho_t) + std::ldexp(std::fabs(cx) + std::fabs(cy) + rho_r + rho_t, -49) + 1e-300;
}

// Error bound of the matrix-pipe screen's squared distances: |S~ - S| <= mx_e2(rho_a, rho_b), with rho_a (rho_b) the largest
// distance of a reference (target) point from the rotation centre, R = rho_a + rho_b, u = 2^-24.  In the kernel's scaled
// units (larger radius in [256, 512)) the screened value of a point pair is
//     S~ = fl_acc( |a~|^2~ + n2(b) - 2 a~ . b~' ),   a~ = a1 + a2, b~' = b1' + b2' the f16 hi + lo splits of a and of R32(b),
// the products exact in fp32 (11 x 11 bits), and the budget is (every term in units of u):
//   * split of both points -- |a - a~|, |b' - b~'| <= 2^-22 |.| per coordinate (two roundings of relative size 2^-11), or
//     2^-14 absolute where a lo piece falls into f16's subnormal range and the matrix pipe flushes it; the distance moves by
//     2 |a - b| (|da| + |db|) <= 2 R sqrt(2) 2^-22 R = 11.3 R^2, with the absolute form 2 R 2 sqrt(2) 2^-14 = 22.6 R^2 (256 / R)
//     <= 22.6 R^2 because the larger radius is at least 256:                                                        23 R^2
//   * the row norm |a~|^2: two f32 roundings (2 rho_a^2), its own split n2 = 256 nh + nl (nh to 0.25, nl to 2^-6 absolute
//     = 4 u rho^2 at rho = 256, less above):                                                                        6 rho_a^2
//   * the column norm is taken from the UNROTATED target point, once per work item: the same 6, the f32 rotation (cos / sin
//     tables rounded to f32: |c^2 + s^2 - 1| <= 1.5 u; two fma per coordinate: |b' - R b| <= 2 sqrt(2) u rho_b) keeps
//     |b|^2 to 9, and the split of the rotated point moves |b'|^2 by 2 rho_b sqrt(2) 2^-22 rho_b = 11.3:               27 rho_b^2
//   * twelve fp32 accumulations inside the MFMA, rounding mode and order unspecified: 2 u each on partial sums that stay
//     below (|a| + |b|)^2 <= R^2:                                                                                   24 R^2
// Sum: u (47 R^2 + 6 rho_a^2 + 27 rho_b^2) -- 55 u R^2 for equal radii.  (Rounds 3 shipped a flat 128 u R^2; the directed
// search of tests/test_gpu_mx_error_bound.py -- coordinates on f16 ties, radii at both edges of the scale, far outliers,
// subnormal lo pieces, tile-edge set sizes, the angles whose f32 (cos, sin) is furthest from unit norm -- found at most
// 2.2 % of that, 5 % of this.)  min and max are 1-Lipschitz, so the bound carries over to the screened Hausdorff value.
double mx_e2(double rho_a, double rho_b)
{
    const double u = 5.9604644775390625e-08, R = rho_a + rho_b;
    return u * (47.0 * R * R + 6.0 * rho_a * rho_a + 27.0 * rho_b * rho_b);
}

// The matrix-pipe kernels' scale exponent e: 2^e rmax in [256, 512) (f16 pieces, their doubles and |x|^2 / 256 stay in range)
int mx_scale_exp(double rmax)
{
    int k = 0;
    (void)std::frexp(rmax * (1.0 + 1e-6), &k);   // radius < 2^k
    return 9 - k;
}

// The screen of one pair searched without bound rounds; `multi`, `nct`, `cls`: the matrix pipe's variant (mx_variant) and
// LDS class.  Pairs sort by (screen, multi, nct, cls), and a run of equal ones forms one launch (LevelPlan::groups).
struct PairScreen {
    Screen screen; int multi, nct, cls;
    auto key() const { return std::tie(screen, multi, nct, cls); }
};

// The matrix-pipe screen, chosen PER PAIR (MM_PRECISION_F32_MATRIX, or a bounded search without its bound rounds) for a
// pair of nr, nt points and radii ra, rb: sets of mx_min_points() .. mx_max_points() points (the kernel is instantiated per
// column-tile count, its row-tile count is a run-time operand, larger target sets are cut into column blocks) and radii the
// scale exponent can take; then also *scale_exp and *e2, the error bound of its squared values.  A set of fewer than 64
// points: no f32 screen, every candidate is scored exactly (cheap at that size, and no packed-FMA kernel runs under this
// precision unless a set exceeds mx_max_points()).  Any other pair keeps `outside` (the packed-FMA screen, or in a batch
// whose largest sets exceed that kernel's registers the direct form) and its e2.
PairScreen mx_pair_screen(int nr, int nt, double ra, double rb, Screen outside, int* scale_exp, double* e2)
{
    if (std::min(nr, nt) < mx_min_points() && std::max(nr, nt) <= mx_max_points()) return {Screen::None, 0, 0, 0};
    const double rmax = std::max(ra, rb);
    if (nr < mx_min_points() || nr > mx_max_points() || nt < mx_min_points() || nt > mx_max_points() || !(rmax > 1.0e-30) ||
        !(rmax < 1.0e30))
        return {outside, 0, 0, 0};
    // LDS is sized per launch by the largest reference set of the group: up to 17 row tiles leave room for two workgroups
    // per CU, more than that for one -- two classes, so that one long contour does not halve the occupancy of every other
    // pair's launch
    PairScreen c{Screen::Matrix, 0, 0, (nr + 31) / 32 <= 17 ? 0 : 1};
    mx_variant(nt, &c.nct, &c.multi);
    *scale_exp = mx_scale_exp(rmax);
    *e2 = mx_e2(ra, rb);
    return c;
}

// One plan_level call: its inputs, the plan it fills, and what one step decides for the steps behind it.
struct Planner {
    const std::vector<int32_t>& set_off; const std::vector<int32_t>& set_len;
    const std::vector<double>& set_rho; const std::vector<int32_t>& set_main;
    const std::vector<PairSpec>& pairs;
    LevelPlan& lp;
    bool expanded = false;              // a precision whose screens work on the expanded distance form
    Screen outside = Screen::Direct;    // the screen of a pair the matrix pipe does not take
    bool use_mx = false;                // some pair takes the matrix pipe (or no screen) instead of `outside`
    std::vector<PairScreen> screen;     // per pair
    int apb = 1; int64_t apb_fill = 1;  // candidates per work item: the batch's, and what fills 24 workgroups per CU
    std::vector<int> pair_group;        // per pair: candidates per group of the culled screen (1: none)
    std::vector<int> order;             // the pairs in work-list order
    std::vector<int64_t> wstart;        // first work item of order[q]; [P]: their number

    double rho_ref(int p) const { return set_rho[(size_t)pairs[(size_t)p].ref_set]; }
    double rho_tgt(int p) const { return set_rho[(size_t)pairs[(size_t)p].tgt_set]; }
    bool searched(int p) const { return !lp.trivial[(size_t)p] && lp.host_pairs[(size_t)p].n_ang != 0; }

    void choose_precision(int precision);
    int describe_pairs(int32_t angle_begin, int32_t angle_end);
    void choose_bound_rounds();
    int choose_screens();
    int apb_of(int p) const;
    int apb_grouped(int p) const;
    void choose_groups();
    int fill_work_list();
    void form_launch_groups();
    void build_bound_work();
    void lay_out();
};

// Non-finite (or overflowing) coordinates: the reference's metric skips the points whose distances are not finite
// (process_utils.rs:112-114) and carries on.  The exact kernels do the same; a screen cannot bound such values, so
// every candidate of this level is scored exactly.  (rho = inf marks such a set, see stage_sets / k_build_sets.)
// The same for finite coordinates an f32 screen cannot hold: squared distances reach (rho_r + rho_t)^2, which must
// stay below FLT_MAX (rho < 1e18 leaves a factor 1e2), and the error bounds of the screens (relative to rho) assume
// that u * rho^2 is far above the f32 denormals (rho > 1e-15 leaves a factor 1e8); rho == 0 (all points at the
// centre) is exact in any format.
void Planner::choose_precision(int precision)
{
    auto f32_safe = [](double rho) { return rho < 1.0e18 && (rho == 0.0 || rho > 1.0e-15); };
    if (precision != MM_PRECISION_F64)
        for (const PairSpec& sp : pairs)
            if (sp.ref_set >= 0 && sp.tgt_set >= 0 && (size_t)sp.ref_set < set_rho.size() && (size_t)sp.tgt_set < set_rho.size() &&
                (!f32_safe(set_rho[sp.ref_set]) || !f32_safe(set_rho[sp.tgt_set]) || !std::isfinite(sp.cx) || !std::isfinite(sp.cy))) {
                precision = MM_PRECISION_F64;
                break;
            }
    lp.precision = precision;
    expanded = precision == MM_PRECISION_F32_FAST || precision == MM_PRECISION_F32_BOUNDED || precision == MM_PRECISION_F32_MATRIX;
}

// The descriptors of the pairs, their slices of the candidate axis and the candidate tables, shared between pairs with the
// same list; then whether the packed-FMA kernel can take the batch.
int Planner::describe_pairs(int32_t angle_begin, int32_t angle_end)
{
    const int P = lp.P;
    lp.host_pairs.assign(P, PairDesc{});
    lp.trivial.assign(P, 0);
    lp.pair_slice_end.assign(P, 0);
    lp.host_tables.clear();
    lp.A = 0; lp.T = 0;
    lp.max_na = 1; lp.max_nbp = 16; lp.max_nt = 1;
    lp.pair_evals = 0.0;
    // table sharing: same list as the previous distinct table (pointer or content) and same slice
    const double* last_ptr = nullptr; int32_t last_n = -1, last_b = -1, last_tab = 0, last_len = -1;
    for (int p = 0; p < P; ++p) {
        const PairSpec& sp = pairs[p];
        if (sp.ref_set < 0 || sp.tgt_set < 0 || (size_t)sp.ref_set >= set_len.size() || (size_t)sp.tgt_set >= set_len.size())
            return set_error(MM_ERR_INVALID, "pair references a set that was not staged");
        if (sp.n_angles < 0) return set_error(MM_ERR_INVALID, "negative candidate count");
        const int32_t nr = set_len[sp.ref_set], nt = set_len[sp.tgt_set];
        const int32_t b = std::min(std::max(angle_begin, sp.slice_begin), sp.n_angles);
        const int32_t en = std::min(std::min(angle_end, sp.slice_end), sp.n_angles);
        const int32_t na = std::max(en - b, 0);
        lp.pair_slice_end[p] = std::max(en, b);
        PairDesc& d = lp.host_pairs[p];
        d.ref_off = set_off[sp.ref_set]; d.n_ref = nr;
        d.tgt_off = set_off[sp.tgt_set]; d.n_tgt = nt;
        d.out_off = (int32_t)lp.A; d.n_ang = na;
        d.ang_full = sp.n_angles; d.ang_begin = b;
        d.n_slice = na; d.pad0 = 0;
        d.flags = sp.flags;
        d.cx = sp.cx; d.cy = sp.cy;
        d.tol2 = sp.tie_tol;
        d.delta = (lp.precision != MM_PRECISION_F64)
                      ? screen_delta(set_rho[sp.ref_set], set_rho[sp.tgt_set], sp.cx, sp.cy) + sp.delta_extra : 0.0;
        {   // expanded-form screening: |d2_f32 - d2| <= 5 u (rho_a + rho_b)^2; we use 8 u (..)^2
            const double rs = set_rho[sp.ref_set] + set_rho[sp.tgt_set];
            d.e2 = expanded ? 8.0 * 5.9604644775390625e-08 * rs * rs : 0.0;
            d.rho_t = set_rho[sp.tgt_set];
        }
        if (nr == 0 || nt == 0) {
            // process_utils.rs:86-88: an empty set makes every cost 0.0 -> the first candidate wins;
            // nothing to launch for this pair (one table entry keeps its first angle).
            lp.trivial[p] = 1;
            d.n_ang = 0;
            d.tab_off = (int32_t)lp.host_tables.size();
            if (na > 0) lp.host_tables.push_back(sp.angles[b]);
            last_ptr = nullptr; last_len = -1;
            continue;
        }
        const bool share = (na == last_len && b == last_b && sp.n_angles == last_n) &&
                           (sp.angles == last_ptr ||
                            (na > 0 && std::memcmp(sp.angles + b, lp.host_tables.data() + last_tab, (size_t)na * 8) == 0));
        if (!share) {
            last_tab = (int32_t)lp.host_tables.size();
            lp.host_tables.insert(lp.host_tables.end(), sp.angles + b, sp.angles + b + na);
            last_len = na; last_b = b; last_n = sp.n_angles;
        }
        last_ptr = sp.angles;
        d.tab_off = last_tab;
        lp.A += na;
        lp.max_na = std::max<int>(lp.max_na, nr);
        lp.max_nbp = std::max<int>(lp.max_nbp, (nt + 15) & ~15);
        lp.max_nt = std::max<int>(lp.max_nt, nt);
        lp.pair_evals += 2.0 * (double)nr * (double)nt * (double)na;
        if (lp.A > (int64_t)1 << 30) return set_error(MM_ERR_TOO_LARGE, "batch exceeds 2^30 candidates");
    }
    lp.T = (int64_t)lp.host_tables.size();
    // the fast screening kernel keeps one row block in registers; bigger sets use the direct form
    lp.use_fast = expanded && lp.max_na <= max_rows_fast() && lp.max_nbp <= max_target_points_fast();
    if (expanded && !lp.use_fast)
        for (PairDesc& d : lp.host_pairs) d.e2 = 0.0;
    return MM_OK;
}

// Whether the bound rounds of MM_PRECISION_F32_BOUNDED run, and on which pipe.
void Planner::choose_bound_rounds()
{
    const int P = lp.P;
    // the bound rounds pay for themselves on sets of a few dozen points or more and on batches that keep
    // the device busy for several rounds of workgroups (a dozen dependent launches cost more than
    // screening a small batch outright: the between stage's 2 x 722 candidates are 40 % faster without);
    // per-candidate costs need every candidate evaluated
    lp.use_lb = lp.precision == MM_PRECISION_F32_BOUNDED && lp.use_fast && !lp.want_costs && lp.A > 0 &&
                lp.A >= lp.opts.bound_min_candidates && std::min(lp.max_na, lp.max_nt) >= 64 &&
                std::max(lp.max_na, lp.max_nt) <= lb_max_points();
    // The bound rounds on the matrix pipe (k_bound_mx) and the survivors through k_screen_mx: every non-trivial pair with
    // sets of 64 .. lb_mx_max_points() points and a radius f16 can be scaled to; the pairs then carry the scale exponent and
    // the matrix kernels' error bound (the larger of the two directions': pass 1 rotates reference queries against target
    // rows, pass 2 target queries against reference rows).  The two per-pair picks stay on the packed-FMA screen (it emits
    // the row / column minima the third round's query choice needs); its e2 is the smaller one.
    lp.lb_mx_tiles = 0; lp.kept_nct = 0; lp.kept_acap = 0;
    if (!lp.use_lb || !lp.opts.bound_matrix) return;
    bool ok = true;
    int tiles = 1, nct0 = -1, acap = 1;
    for (int p = 0; p < P && ok; ++p) {
        const PairDesc& d = lp.host_pairs[p];
        if (!searched(p)) continue;
        const double rmax = std::max(rho_ref(p), rho_tgt(p));
        ok = d.n_ref >= mx_min_points() && d.n_tgt >= mx_min_points() && d.n_ref <= lb_mx_max_points() &&
             d.n_tgt <= lb_mx_max_points() && rmax > 1.0e-30 && rmax < 1.0e30;
        tiles = std::max(tiles, (std::max(d.n_ref, d.n_tgt) + 31) / 32);
        int nct = 0, multi = 0;
        mx_variant(d.n_tgt, &nct, &multi);
        if (multi) nct = 0;
        nct0 = nct0 < 0 ? nct : (nct0 == nct ? nct0 : 0);     // 0: the pairs do not share one variant
        acap = std::max(acap, (d.n_ref + 31) / 32);
    }
    // The picks and the survivors go through k_screen_mx from device queues, which takes ONE variant per launch: every
    // pair must have the same column-tile count (and <= 17 row tiles, two workgroups per CU).  (k_screen_mx gives a
    // candidate to one wave, ~10 us, where the packed-FMA screen spends 2 - 3 us of a whole workgroup -- 222 against
    // 156 us per step for config3's survivors -- but the packed-FMA kernels are not to run beside MFMA kernels:
    // profiles/README.md, "packed-FMA kernels beside MFMA kernels".)  A batch of mixed shapes, or one with sets beyond
    // the bound kernel's range, is screened outright on the matrix pipe instead.
    ok = ok && nct0 > 0 && acap <= 17;
    if (!ok) { lp.use_lb = false; return; }
    lp.lb_mx_tiles = tiles;
    lp.kept_nct = nct0; lp.kept_acap = acap;
    for (int p = 0; p < P; ++p) {
        PairDesc& d = lp.host_pairs[p];
        if (!searched(p)) continue;
        const double ra = rho_ref(p), rb = rho_tgt(p);
        d.pad0 = mx_scale_exp(std::max(ra, rb));
        d.e2 = std::max(mx_e2(ra, rb), mx_e2(rb, ra));
    }
}

// The screen of every pair searched without bound rounds.  A bounded search that does not run its bound rounds (small batch,
// per-candidate costs asked for, sets outside the bound kernel's range) screens every candidate: on the matrix pipe, like
// MM_PRECISION_F32_MATRIX.
int Planner::choose_screens()
{
    const bool mx_wanted = lp.precision == MM_PRECISION_F32_MATRIX || (lp.precision == MM_PRECISION_F32_BOUNDED && !lp.use_lb);
    use_mx = false;
    outside = lp.use_fast ? Screen::PackedFma : Screen::Direct;
    screen.assign((size_t)lp.P, PairScreen{outside, 0, 0, 0});
    if (mx_wanted && lp.A > 0) {
        for (int p = 0; p < lp.P; ++p) {
            PairDesc& d = lp.host_pairs[p];
            if (!searched(p)) continue;
            screen[(size_t)p] = mx_pair_screen(d.n_ref, d.n_tgt, rho_ref(p), rho_tgt(p), outside, &d.pad0, &d.e2);
            use_mx = use_mx || screen[(size_t)p].screen != outside;
        }
    }
    if (lp.max_nbp > max_target_points_f64() || (lp.precision != MM_PRECISION_F64 && lp.max_nbp > max_target_points_f32()))
        return set_error(MM_ERR_TOO_LARGE, "target set does not fit the kernel's LDS budget (" +
                                               std::to_string(max_target_points_f64()) + " points)");
    return MM_OK;
}

// ---- work decomposition: one work item = `apb` consecutive candidates of one pair ----
// With the matrix-pipe screen more of them: a work item of the FULL kernel (k_screen_mx) stages the pair's rows once (global
// loads, two barriers: ~3 us, with one other workgroup on the CU to hide it) and a 17 x 17-tile candidate takes a wave
// 10 us, a 7 x 7 one 1.8.  A wave should see ~2300 tiles per item (17 x 17 tiles: 8 candidates, 32 per workgroup; small sets
// up to 16 per wave) as far as the batch has candidates for 24 workgroups per CU: config3's launch 16.19 ms at 578 tiles,
// 16.00 at 1156, 15.83 at 2312, 15.77 at 4624 (tools/exp_apb.sh, on the full kernel).
// The CULLED kernel keeps the item size (the groups of eight candidates and the waves' shares hang on it) but computes
// 40.45 of the 289 tiles of such a candidate: a wave sees ~320 tiles per item, and the item's prologue -- rows, target points,
// norms and 34 bounding circles, each circle by one thread -- is larger than the full kernel's.  That is paid per RUN of
// items instead (plan_runs below): a workgroup keeps its pair for up to five items of config3's launch.
int Planner::apb_of(int p) const
{
    if (screen[(size_t)p].screen != Screen::Matrix) return apb;
    const PairDesc& d = lp.host_pairs[p];
    const int64_t tiles = (int64_t)((d.n_ref + 31) / 32) * ((d.n_tgt + 31) / 32);
    const int64_t per_wave = std::min<int64_t>(16, std::max<int64_t>(2, (2312 + tiles - 1) / tiles));
    return (int)std::max<int64_t>(apb, std::min<int64_t>(4 * per_wave, apb_fill));
}

int Planner::apb_grouped(int p) const
{
    const int g = pair_group[(size_t)p];
    return g > 1 ? std::max(apb_of(p), 4 * g) : apb_of(p);
}

// The batch's candidates per work item, and the culled screen's groups (ScreenOptions::screen_group): per pair the
// candidates that share one tile bound.  A forced size asks for work items of four groups, one per wave; the automatic one
// follows the pair's list and never takes more than a quarter of the item the batch gives the pair, so that a small batch
// keeps a candidate per wave.
void Planner::choose_groups()
{
    const int64_t target_wgs = 256 * 24;
    // the packed-FMA and exact kernels: at most 8 candidates per workgroup, measured on config3 (apb 2/4/8/16/64/128: 140.6/145.0/146.3/
    // 144.6/138.2/122.3 TFLOP/s) -- many short workgroups keep the co-resident ones out of phase
    // (rotation / epilogue of one overlaps the micro-tile loop of the others) and balance the tail
    apb = (int)std::min<int64_t>(8, std::max<int64_t>(1, (lp.A + target_wgs - 1) / target_wgs));
    // matrix-pipe screen: one WAVE per candidate, four waves per workgroup -- a workgroup of fewer than four candidates
    // leaves waves idle for the whole item (small batches: a single search of 361 candidates)
    if (use_mx) apb = std::max(apb, 4);
    apb_fill = std::max<int64_t>(1, (lp.A + target_wgs - 1) / target_wgs);
    pair_group.assign((size_t)lp.P, 1);
    if (!(use_mx && lp.opts.screen_cull && lp.opts.screen_group != 1)) return;
    int32_t seen_tab = -1, seen_n = -1; int seen_g = 1;
    for (int p = 0; p < lp.P; ++p) {
        const PairScreen& c = screen[(size_t)p];
        const PairDesc& d = lp.host_pairs[p];
        if (c.screen != Screen::Matrix || c.multi || d.n_ang < 2) continue;
        const int gmax = mx_cull_group_max(c.nct);
        if (gmax < 2) continue;
        int g = lp.opts.screen_group;
        if (g == 0) {
            if (d.tab_off != seen_tab || d.n_ang != seen_n) {
                seen_g = mm_tile_group_auto(lp.host_tables.data() + d.tab_off, d.n_ang);
                seen_tab = d.tab_off; seen_n = d.n_ang;
            }
            g = seen_g;
            while (g > 1 && 4 * g > apb_of(p)) g >>= 1;
        }
        pair_group[(size_t)p] = std::min(g, gmax);
    }
}

// balanced chunks: ceil(n / apb) workgroups whose sizes differ by at most one (a 90-candidate
// slice is 12 x 7-8 candidates, not 11 x 8 + 2: the short tail would cost a full staging).
// 186 k items for config3: sized by a prefix sum and filled over the worker pool (one push_back at a time
// this was half of a case's staging time).  With the matrix-pipe screen the pairs are laid out group by group
// (stable: pair-major inside a group, as the XCD-aware work order wants it).
int Planner::fill_work_list()
{
    const int P = lp.P;
    order.resize((size_t)P);
    for (int p = 0; p < P; ++p) order[(size_t)p] = p;
    if (use_mx) std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return screen[(size_t)x].key() < screen[(size_t)y].key(); });
    wstart.assign((size_t)P + 1, 0);
    for (int q = 0; q < P; ++q) {
        const int ap = apb_grouped(order[(size_t)q]);
        wstart[(size_t)q + 1] = wstart[(size_t)q] + (lp.host_pairs[order[(size_t)q]].n_ang + ap - 1) / ap;
    }
    if (wstart[(size_t)P] > INT32_MAX) return set_error(MM_ERR_TOO_LARGE, "too many work items");
    lp.host_work.resize((size_t)wstart[(size_t)P]);
    WorkItem* hw = lp.host_work.data();
    constexpr int kBlk = 64;
    parallel_for((P + kBlk - 1) / kBlk, [&](int blk) {
        for (int q = blk * kBlk; q < std::min(P, (blk + 1) * kBlk); ++q) {
            const int p = order[(size_t)q];
            const PairDesc& d = lp.host_pairs[p];
            const int nw = (int)(wstart[(size_t)q + 1] - wstart[(size_t)q]);
            WorkItem* o = hw + wstart[(size_t)q];
            for (int k = 0; k < nw; ++k) {
                const int a0 = (int)((int64_t)d.n_ang * k / nw), a1 = (int)((int64_t)d.n_ang * (k + 1) / nw);
                o[k] = WorkItem{p, a0, a1 - a0, pair_group[(size_t)p] > 1 ? pair_group[(size_t)p] : 0};
            }
        }
    });
    lp.W = (int)lp.host_work.size();
    return MM_OK;
}

// one launch per run of pairs with the same screen; a matrix group takes the culled kernel if it can
void Planner::form_launch_groups()
{
    const int P = lp.P;
    lp.groups.clear();
    lp.host_runs.clear();
    if (lp.precision == MM_PRECISION_F64 || lp.use_lb) return;
    for (int q = 0; q < P;) {
        const PairScreen c = screen[(size_t)order[(size_t)q]];
        ScreenGroup g{c.screen, c.nct, c.multi, 1, (int)wstart[(size_t)q], 0, 0, 0};
        int q1 = q;
        for (; q1 < P && screen[(size_t)order[(size_t)q1]].key() == c.key(); ++q1) {
            const PairDesc& d = lp.host_pairs[order[(size_t)q1]];
            if (d.n_ang > 0) g.a_cap = std::max(g.a_cap, (d.n_ref + 31) / 32);
            g.candidates += d.n_ang;
            g.tiles_full += (int64_t)d.n_ang * ((d.n_ref + 31) / 32) * c.nct;
        }
        g.work_count = (int)(wstart[(size_t)q1] - wstart[(size_t)q]);
        if (g.screen == Screen::Matrix && lp.opts.screen_cull && mx_cull_takes(g.nct, g.multi, g.a_cap)) g.screen = Screen::MatrixCull;
        // the culled screen lays a set of two runs out run by run where that adds no tile: per set, per pair side
        if (g.screen == Screen::MatrixCull && lp.opts.screen_split)
            for (int k = q; k < q1; ++k) {
                const int p = order[(size_t)k];
                PairDesc& d = lp.host_pairs[p];
                d.ref_main = mm_tile_split_main(d.n_ref, set_main[(size_t)pairs[p].ref_set]);
                d.tgt_main = mm_tile_split_main(d.n_tgt, set_main[(size_t)pairs[p].tgt_set]);
            }
        // the culled screen's runs: a workgroup keeps its pair for consecutive items (plan_runs)
        if (g.screen == Screen::MatrixCull && g.work_count > 0) {
            g.run_begin = (int)lp.host_runs.size();
            g.run_count = plan_runs(lp.host_work.data() + g.work_begin, g.work_count, lp.opts.screen_run, lp.host_runs);
        }
        if (g.work_count > 0) lp.groups.push_back(g);
        q = q1;
    }
}

// The first bound round's work list and the sizes of the rounds behind it.
void Planner::build_bound_work()
{
    lp.host_work_lb.clear();
    lp.W_lb = 0; lp.lb_runs_cap = 0; lp.lb_pair_evals = 0.0; lp.lb_sparse_total = 0;
    if (!lp.use_lb) return;
    // every lb_stride-th point of either set is a query; the subset has to fit the kernel's registers
    const int qmax = lp.kept_nct > 0 ? 32 * lp.opts.bound_matrix_qt : lb_max_query_points();
    lp.lb_stride = std::max(lp.kept_nct > 0 ? 1 : 8, (std::max(lp.max_na, lp.max_nt) + qmax - 1) / qmax);
    // first round: every lb_candidate_step()-th candidate and the last one, 32 of them per workgroup
    // (4 waves x 8: amortises staging the reference set)
    const int apb_lb = 32, cstep = lb_candidate_step();
    for (int p = 0; p < lp.P; ++p) {
        const PairDesc& d = lp.host_pairs[p];
        const int ne = lb_sparse_candidates(d.n_ang);
        for (int i0 = 0; i0 < ne; i0 += apb_lb)
            lp.host_work_lb.push_back(WorkItem{p, i0 * cstep, std::min(apb_lb, ne - i0), cstep});
        lp.lb_runs_cap += (d.n_ang + 7) / 8;
        const double qa = (d.n_ref + lp.lb_stride - 1) / lp.lb_stride, qb = (d.n_tgt + lp.lb_stride - 1) / lp.lb_stride;
        lp.lb_pair_evals += (qa * d.n_tgt + qb * d.n_ref) * (double)ne;
        lp.lb_sparse_total += ne;
    }
    lp.W_lb = (int)lp.host_work_lb.size();
}

// The regions of the level blob, in the order they lie (LevelLayout).
void Planner::lay_out()
{
    LevelLayout& l = lp.lay;
    const size_t P = (size_t)lp.P, A = (size_t)lp.A, T = (size_t)lp.T;
    const bool use_lb = lp.use_lb;
    size_t o = 0;
    auto take = [&](size_t bytes) { const size_t at = o; o = align_up(o + std::max<size_t>(bytes, 16)); return at; };
    l.pairs = take(P * sizeof(PairDesc));
    l.work = take((size_t)lp.W * sizeof(WorkItem));
    l.work_lb = take((size_t)lp.W_lb * sizeof(WorkItem));
    l.cos32 = take(T * 4); l.sin32 = take(T * 4);
    l.cos64 = take(T * 8); l.sin64 = take(T * 8); l.ang64 = take(T * 8);
    l.runs = lp.host_runs.empty() ? 0 : take(lp.host_runs.size() * sizeof(WorkRun));
    l.lvl_in_bytes = o;
    l.sq32 = take(A * 4); l.sq64 = take(A * 8); l.flag = take(A);
    l.items = take(A * sizeof(WorkItem)); l.n_items = take(32);
    l.emit_rows = (lp.max_na + 3) & ~3; l.emit_cols = (lp.max_nt + 3) & ~3;
    l.lb32 = take(use_lb ? A * 4 : 0); l.pick = take(use_lb ? P * 8 : 0);
    l.items_pick = take(use_lb ? P * 2 * sizeof(WorkItem) : 0);
    l.items_lb = take(use_lb ? (size_t)lp.lb_runs_cap * 3 * sizeof(WorkItem) : 0);
    l.klist = take(lp.kept_nct > 0 ? A * 4 : 0);
    l.emit = take(use_lb ? P * (size_t)(l.emit_rows + l.emit_cols) * 4 : 0);
    l.qlist = take(use_lb ? P * 2 * (size_t)lb_list_queries() * 4 : 0);
    l.best_cost = take(P * 8); l.best_idx = take(P * 4); l.n_rescored = take(P * 4);
    l.near_cnt = take(P * 4); l.near_idx = take(P * 4 * kMaxNear);
    l.off_best_cost = l.best_cost; l.res_bytes = o - l.best_cost;
    l.off_all_costs = lp.want_costs ? take(A * 8) : 0;
    l.lvl_bytes = o;
    l.r_best_idx = l.best_idx - l.best_cost; l.r_n_rescored = l.n_rescored - l.best_cost;
    l.r_near_cnt = l.near_cnt - l.best_cost; l.r_near_idx = l.near_idx - l.best_cost;
}

}  // namespace

int plan_runs(const WorkItem* w, int n, int run, std::vector<WorkRun>& out)
{
    if (run == 1 || run < 0 || n <= 0) return 0;
    const int cap = run ? run : n / (kRunMinRounds * kRunResidentWgs);
    if (cap < 2) return 0;
    const size_t before = out.size();
    for (int i = 0; i < n;) {
        const int want = run ? cap : std::min(cap, std::max(1, (n - i + 2 * kRunResidentWgs - 1) / (2 * kRunResidentWgs)));
        int e = i + 1;
        while (e < n && e - i < want && w[e].pair == w[i].pair) ++e;
        out.push_back(WorkRun{i, e - i});
        i = e;
    }
    return (int)(out.size() - before);
}

int plan_level(const std::vector<int32_t>& set_off, const std::vector<int32_t>& set_len, const std::vector<double>& set_rho,
               const std::vector<int32_t>& set_main, const std::vector<PairSpec>& pairs, int precision, int32_t angle_begin,
               int32_t angle_end, bool want_costs, const ScreenOptions& opts, LevelPlan& out)
{
    out.opts = opts;
    out.precision = precision;
    out.want_costs = want_costs;
    out.slice_end = angle_end;
    out.P = (int)pairs.size();
    if (precision != MM_PRECISION_F64 && precision != MM_PRECISION_F32 && precision != MM_PRECISION_F32_FAST &&
        precision != MM_PRECISION_F32_BOUNDED && precision != MM_PRECISION_F32_MATRIX)
        return set_error(MM_ERR_INVALID, "precision must be MM_PRECISION_F64, MM_PRECISION_F32, MM_PRECISION_F32_FAST, "
                                         "MM_PRECISION_F32_BOUNDED or MM_PRECISION_F32_MATRIX");
    Planner pl{set_off, set_len, set_rho, set_main, pairs, out};
    pl.choose_precision(precision);
    if (angle_begin < 0) angle_begin = 0;
    int rc;

    TraceTimer tt_desc("stage_level: descriptors");
    if ((rc = pl.describe_pairs(angle_begin, angle_end))) return rc;
    pl.choose_bound_rounds();
    if ((rc = pl.choose_screens())) return rc;
    tt_desc.stop();

    TraceTimer tt_work("stage_level: work list");
    pl.choose_groups();
    if ((rc = pl.fill_work_list())) return rc;
    pl.form_launch_groups();
    pl.build_bound_work();
    tt_work.stop();

    pl.lay_out();
    return MM_OK;
}

void serialize_level_plan(const LevelPlan& lp, std::vector<int64_t>& w)
{
    auto bits = [](double v) { int64_t b; std::memcpy(&b, &v, 8); return b; };
    const LevelLayout& l = lp.lay;
    const ScreenOptions& op = lp.opts;
    const int64_t header[] = {lp.precision, lp.P, lp.W, lp.W_lb, lp.A, lp.T, lp.max_na, lp.max_nbp, lp.max_nt, lp.use_fast, lp.use_lb,
                              lp.lb_stride, lp.lb_runs_cap, lp.lb_mx_tiles, lp.kept_nct, lp.kept_acap, bits(lp.pair_evals),
                              bits(lp.lb_pair_evals), lp.lb_sparse_total, lp.slice_end, lp.want_costs, op.bound_min_candidates,
                              op.bound_matrix, op.bound_matrix_qt, op.bound_matrix_nc, op.screen_cull, op.screen_split, op.screen_group};
    const size_t layout[] = {l.pairs, l.work, l.work_lb, l.cos32, l.sin32, l.cos64, l.sin64, l.ang64, l.sq32, l.sq64, l.flag, l.items,
                             l.n_items, l.lb32, l.pick, l.items_pick, l.items_lb, l.klist, l.emit, l.qlist, l.best_cost, l.best_idx,
                             l.n_rescored, l.near_cnt, l.near_idx, l.lvl_in_bytes, l.lvl_bytes, l.off_best_cost, l.res_bytes,
                             l.off_all_costs, l.r_best_idx, l.r_n_rescored, l.r_near_cnt, l.r_near_idx, (size_t)l.emit_rows,
                             (size_t)l.emit_cols};
    w.clear();
    w.push_back((int64_t)(sizeof header / sizeof header[0]));
    w.insert(w.end(), std::begin(header), std::end(header));
    w.push_back((int64_t)(sizeof layout / sizeof layout[0]));
    for (size_t v : layout) w.push_back((int64_t)v);
    w.push_back(22 * (int64_t)lp.P);
    for (int p = 0; p < lp.P; ++p) {
        const PairDesc& d = lp.host_pairs[(size_t)p];
        const int64_t rec[22] = {d.ref_off, d.n_ref, d.tgt_off, d.n_tgt, d.tab_off, d.out_off, d.n_ang, d.flags, d.ang_full, d.ang_begin,
                                 d.n_slice, d.pad0, d.ref_main, d.tgt_main, bits(d.cx), bits(d.cy), bits(d.delta), bits(d.tol2),
                                 bits(d.e2), bits(d.rho_t), lp.trivial[(size_t)p], lp.pair_slice_end[(size_t)p]};
        w.insert(w.end(), rec, rec + 22);
    }
    w.push_back((int64_t)lp.host_tables.size());
    for (double t : lp.host_tables) w.push_back(bits(t));
    for (const std::vector<WorkItem>* list : {&lp.host_work, &lp.host_work_lb}) {
        w.push_back(4 * (int64_t)list->size());
        for (const WorkItem& it : *list) { const int64_t rec[4] = {it.pair, it.a0, it.cnt, it.pad}; w.insert(w.end(), rec, rec + 4); }
    }
    w.push_back(8 * (int64_t)lp.groups.size());
    for (const ScreenGroup& g : lp.groups) {
        const int64_t rec[8] = {(int64_t)g.screen, g.nct, g.multi, g.a_cap, g.work_begin, g.work_count, g.candidates, g.tiles_full};
        w.insert(w.end(), rec, rec + 8);
    }
}

}  // namespace mm
