// mm_branch.cpp -- CCTA branch labelling (include/mm_ccta.h): the branches of a centerline within reach of every mesh
// point in one device pass (mm_branch_kernels.hip), and the main / side / per-side-branch lists of label_branches
// (multimodars/ccta/labeling.py:415-487) read off those masks on the host.
#include <algorithm>
#include <climits>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/mm_ccta.h"
#include "mm_stage.h"

namespace mm {
namespace {

int branch_masks(mm_engine* h, const mm_clpoint* cl, int64_t ncl, const double* pts, int64_t n, double radius,
                 uint64_t* masks, const char* who)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (n <= 0 || ncl <= 0 || !cl || !pts || !masks) return set_error(MM_ERR_INVALID, std::string(who) + ": bad arguments");
    if (n > INT32_MAX || ncl > INT32_MAX / 64)
        return set_error(MM_ERR_TOO_LARGE, std::string(who) + ": too many points for one pass");
    for (int64_t k = 0; k < ncl; ++k)
        if (cl[k].branch_id >= MM_BRANCH_MASK_BITS)
            return set_error(MM_ERR_INVALID, std::string(who) + ": branch_id " + std::to_string(cl[k].branch_id) +
                                                 " does not fit a mask of " + std::to_string(MM_BRANCH_MASK_BITS) + " branches");
    StagedPass sp;
    const size_t o_pts = sp.in.take((size_t)n * 24), o_cl = sp.in.take((size_t)ncl * sizeof(BranchClPoint));
    const size_t o_mask = sp.out.take((size_t)n * 8);
    if ((rc = sp.reserve(e))) return rc;
    std::memcpy(sp.host<double>(o_pts), pts, (size_t)n * 24);
    BranchClPoint* hc = sp.host<BranchClPoint>(o_cl);
    for (int64_t k = 0; k < ncl; ++k) hc[k] = BranchClPoint{cl[k].x, cl[k].y, cl[k].z, 1ull << cl[k].branch_id};
    rc = sp.run((double)n * (double)ncl, "branch mask launch", [&] {
        return launch_branch_mask(sp.dev_in<double>(o_pts), n, sp.dev_in<BranchClPoint>(o_cl), (int)ncl,
                                  radius * radius,   // label_coronary.rs:226
                                  sp.dev_out<unsigned long long>(o_mask), e->stream);
    });
    if (rc) return rc;
    std::memcpy(masks, sp.host<uint64_t>(o_mask), (size_t)n * 8);
    return MM_OK;
}

int branch_select(const uint64_t* masks, int64_t n, const uint32_t* main_ids, int64_t n_main, int64_t n_branches,
                  int64_t* main_idx, int64_t* side_idx, int64_t* side_k_off, int64_t* side_k_idx, int64_t side_k_cap,
                  int64_t* counts, const char* who)
{
    if (n < 0 || n_main < 0 || n_branches < 0 || n_branches > MM_BRANCH_MASK_BITS || side_k_cap < 0 || !counts ||
        !side_k_off || (n > 0 && !masks) || (n_main > 0 && !main_ids))
        return set_error(MM_ERR_INVALID, std::string(who) + ": bad arguments");
    uint64_t main = 0;
    for (int64_t k = 0; k < n_main; ++k) {
        if (main_ids[k] >= MM_BRANCH_MASK_BITS) return set_error(MM_ERR_INVALID, std::string(who) + ": a main branch id does not fit the mask");
        main |= (uint64_t)1 << main_ids[k];
    }
    int64_t nm = 0, ns = 0;
    std::vector<int64_t> per((size_t)n_branches, 0);
    for (int64_t i = 0; i < n; ++i) {
        if (masks[i] & main) { if (main_idx) main_idx[nm] = i; ++nm; continue; }           // labeling.py:465
        if (side_idx) side_idx[ns] = i;                                                    // :466
        ++ns;
        for (uint64_t m = masks[i]; m; m &= m - 1) {
            const int b = __builtin_ctzll(m);
            if (b < n_branches) ++per[(size_t)b];
        }
    }
    side_k_off[0] = 0;
    for (int64_t b = 0; b < n_branches; ++b) side_k_off[b + 1] = side_k_off[b] + per[(size_t)b];   // main branches: empty
    counts[0] = nm; counts[1] = ns; counts[2] = side_k_off[n_branches];
    if (side_k_idx && counts[2] <= side_k_cap) {                                           // :479-484 side_k = the side points near k
        std::vector<int64_t> at(side_k_off, side_k_off + n_branches);
        for (int64_t i = 0; i < n; ++i) {
            if (masks[i] & main) continue;
            for (uint64_t m = masks[i]; m; m &= m - 1) {
                const int b = __builtin_ctzll(m);
                if (b < n_branches) side_k_idx[at[(size_t)b]++] = i;
            }
        }
    }
    return MM_OK;
}

}  // namespace
}  // namespace mm

using namespace mm;

extern "C" {

int mm_branch_tile_points(void) { return branch_tile_points(); }

int mm_branch_masks(mm_engine* h, const mm_clpoint* cl, int64_t ncl, const double* pts_xyz, int64_t n, double radius,
                    uint64_t* masks_out)
{
    return branch_masks(h, cl, ncl, pts_xyz, n, radius, masks_out, "mm_branch_masks");
}

int mm_branch_select(const uint64_t* masks, int64_t n, const uint32_t* main_ids, int64_t n_main, int64_t n_branches,
                     int64_t* main_idx, int64_t* side_idx, int64_t* side_k_off, int64_t* side_k_idx, int64_t side_k_cap,
                     int64_t* counts)
{
    return branch_select(masks, n, main_ids, n_main, n_branches, main_idx, side_idx, side_k_off, side_k_idx, side_k_cap,
                         counts, "mm_branch_select");
}

int mm_label_branches(mm_engine* h, const mm_clpoint* cl, int64_t ncl, const double* pts_xyz, int64_t n, double radius,
                      const uint32_t* main_ids, int64_t n_main, int64_t n_branches, uint64_t* masks_out, int64_t* main_idx,
                      int64_t* side_idx, int64_t* side_k_off, int64_t* side_k_idx, int64_t side_k_cap, int64_t* counts)
{
    if (!main_idx || !side_idx || !side_k_off || !counts || n_main < 0 || (n_main > 0 && !main_ids) || n_branches < 0 ||
        n_branches > MM_BRANCH_MASK_BITS || side_k_cap < 0)
        return set_error(MM_ERR_INVALID, "mm_label_branches: bad arguments");
    int rc = branch_masks(h, cl, ncl, pts_xyz, n, radius, masks_out, "mm_label_branches");
    if (rc) return rc;
    return branch_select(masks_out, n, main_ids, n_main, n_branches, main_idx, side_idx, side_k_off, side_k_idx, side_k_cap,
                         counts, "mm_label_branches");
}

}  // extern "C"
