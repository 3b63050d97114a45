// mm_point_device.h -- the nearest entry of a small set, one point per lane: the fold k_slice_nearest
// (mm_slice_kernels.hip) and k_cl_morph (mm_morph_kernels.hip) share.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

namespace mm {

static constexpr int kNearestTile = 512;    // entries of the small set per LDS tile (512 x 32 B = 16 KiB)
static constexpr int kNearestLanes = 256;   // points per work item, one per lane

// The fold of one lane's point (px, py, pz) over the n entries of set (STRIDE doubles each, xyz first), in entry order:
//   d_j = (px - x_j)^2 + (py - y_j)^2 + (pz - z_j)^2      three products, (dx^2 + dy^2) + dz^2, never fused
//   entry j replaces the best iff d_j < best
// so ties keep the lowest index and a NaN d_j is never chosen.  Returns the best entry's index, 0 if no entry beat the
// start value `best`: the caller's start value is the rule for such a point, and each kernel states its own.  Every lane
// of the block must call (two barriers per tile); the entries go through LDS in tiles of kNearestTile as (x, y, z, pad),
// read at the same address by all lanes (broadcast, conflict-free).
template <int STRIDE>
static __device__ __forceinline__ int nearest_fold(const double* set, int n, double px, double py, double pz,
                                                   double best)
{
    int bi = 0;
    __shared__ double4 s_e[kNearestTile];
    const int tid = threadIdx.x;
    for (int t0 = 0; t0 < n; t0 += kNearestTile) {
        const int nt = n - t0 < kNearestTile ? n - t0 : kNearestTile;
        __syncthreads();   // the previous tile is fully consumed
        for (int j = tid; j < nt; j += kNearestLanes) {
            const double* e = set + STRIDE * (size_t)(t0 + j);
            s_e[j] = make_double4(e[0], e[1], e[2], 0.0);
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < nt; ++j) {
            const double4 e = s_e[j];
            const double dx = px - e.x, dy = py - e.y, dz = pz - e.z;
            const double d = dx * dx + dy * dy + dz * dz;
            if (d < best) { best = d; bi = t0 + j; }
        }
    }
    return bi;
}

}  // namespace mm
