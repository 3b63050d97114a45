// mm_branch_kernels.hip -- which branches of a centerline come within a radius of each mesh point, exact f64, for gfx950.
//
// mask[i] bit b <=> some centerline point c of branch b has  dx*dx + dy*dy + dz*dz <= r2  with d = p_i - c and
// r2 = radius * radius formed once on the host: the membership test of find_centerline_bounded_points
// (src/ccta/adjust_mesh/label_coronary.rs:201-235) exactly as k_nn3_count makes it behind mm_centerline_bounded_points
// (mm_nn_kernels.hip: the same operands, the same order, no contraction -- the file is built with -ffp-contract=off).  A
// NaN distance is never within.  label_branches (multimodars/ccta/labeling.py:415-487) asks that question once per
// branch, over the same points; here every (point, centerline point) pair is tested once and the answers of all branches
// leave in one word.
//
// Mapping: one lane = one mesh point, 256 lanes per block; the point's coordinates and its running mask stay in
// registers.  The centerline is the small side: the host packs every point as (x, y, z, 1 << branch_id), 32 bytes, and
// the block stages it through LDS in tiles of kBranchTile; in the inner loop all lanes read the same address (two
// ds_read_b128 broadcasts per centerline point, conflict-free).  Per pair: 3 sub + 3 mul + 2 add + 1 compare in f64 and
// a select + or on the mask, against 2 LDS reads -> bound by fp64 VALU issue, like k_nn3_count.  The mask is written
// once, by a plain 8-byte vector store; no atomics.
//
// No early exit: a lane could stop testing a branch whose bit it already holds, but lanes of a wave sit at different
// places of the mesh and hold different bits, so the skip would need a wave-wide vote per branch segment and a centerline
// sorted by branch, for a kernel whose whole run (N = 2 * 10^5, M = 2000: 4 * 10^8 tests) is shorter than the upload of
// its points.  The loop stays branch-free.
#include <hip/hip_runtime.h>

#include "mm_device.h"

namespace mm {

static constexpr int kBranchTile = 1024;    // centerline points per LDS tile (1024 x 32 B = 32 KiB)
static constexpr int kBranchLanes = 256;    // mesh points per block

// pts: n xyz triples; cl: m packed centerline points; mask: n words
__global__ void __launch_bounds__(256)
k_branch_mask(const double* __restrict__ pts, long long n, const BranchClPoint* __restrict__ cl, int m, double r2,
              unsigned long long* __restrict__ mask)
{
    __shared__ BranchClPoint s_c[kBranchTile];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * kBranchLanes + tid;
    const long long pi = i < n ? i : n - 1;   // lanes past the end recompute the last point, never stored
    const double px = pts[3 * pi], py = pts[3 * pi + 1], pz = pts[3 * pi + 2];
    unsigned long long acc = 0ull;
    for (int t0 = 0; t0 < m; t0 += kBranchTile) {
        const int nt = m - t0 < kBranchTile ? m - t0 : kBranchTile;
        __syncthreads();   // the previous tile is fully consumed
        for (int j = tid; j < nt; j += kBranchLanes) s_c[j] = cl[t0 + j];
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < nt; ++j) {
            const BranchClPoint c = s_c[j];
            const double dx = px - c.x, dy = py - c.y, dz = pz - c.z;
            const double v = dx * dx + dy * dy + dz * dz;
            acc |= v <= r2 ? c.bit : 0ull;
        }
    }
    if (i < n) mask[i] = acc;
}

int branch_tile_points() { return kBranchTile; }

hipError_t launch_branch_mask(const double* pts, long long n, const BranchClPoint* cl, int m, double r2,
                              unsigned long long* mask, hipStream_t s)
{
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_branch_mask, dim3((unsigned)((n + kBranchLanes - 1) / kBranchLanes)), dim3(kBranchLanes), 0, s,
                       pts, n, cl, m, r2, mask);
    return hipGetLastError();
}

}  // namespace mm
