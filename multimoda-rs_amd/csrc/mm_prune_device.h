// mm_prune_device.h -- the device half of the pruned exact-f64 searches (k_nn3_min in mm_nn_kernels.hip, k_tri_min in
// mm_tri_kernels.hip): what an item does with the lower bound lb2 the host gave it (mm_prune.h, box_lb2) and how a lane's
// minimum enters the output.  The output holds the bit patterns of non-negative doubles, pre-filled with +inf: as
// unsigned integers they order like the values, so a minimum is a 64-bit atomicMin; a NaN never enters, because the
// lanes' own folds never take one.  The argument is DESIGN.md 4.20.  Device code only.
#pragma once

#include <hip/hip_runtime.h>

namespace mm {

static constexpr unsigned long long kInfBits = 0x7ff0000000000000ull;   // +inf

// The largest of the block's values v (one per lane), through *s_max in LDS; uniform.  Every lane of the block must
// call: three barriers.  The first keeps the previous item's readers of *s_max ahead of the reset, the second the
// reset ahead of the atomics, the third the atomics ahead of the read.
__device__ __forceinline__ unsigned long long block_max(unsigned long long v, unsigned long long* s_max)
{
    __syncthreads();
    if (threadIdx.x == 0) *s_max = 0ull;
    __syncthreads();
    atomicMax(s_max, v);
    __syncthreads();
    return *s_max;
}

// May an item with bound lb2 be skipped, `top` being the largest current minimum of its query block?  (A stale, larger
// minimum only costs work: the values only decrease.)  Every distance of the item is >= lb2.
//   pass B      lb2 >= top: no distance here is below any of the block's minima, so none can lower one;
//   who pass    lb2 >  top: only then can none EQUAL a final minimum -- an equal distance still wins on face index.
enum class Skip { cannot_lower, cannot_equal };
__device__ __forceinline__ bool skip_item(Skip rule, double lb2, double top)
{
    return rule == Skip::cannot_equal ? lb2 > top : lb2 >= top;
}

// Merges a lane's minimum m into *out.  The stored values only ever decrease, so a (possibly stale) plain read that is
// already <= ours proves the atomic would change nothing: most items of pass B improve few of their queries.
__device__ __forceinline__ void merge_min(unsigned long long* out, unsigned long long m)
{
    if (m < *out) atomicMin(out, m);
}

}  // namespace mm
