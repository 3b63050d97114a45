// mm_xcd.h -- the XCD-aware work order of the kernels that take one workgroup per work item (device code only).
#pragma once

#include <hip/hip_runtime.h>

namespace mm {

// XCD-aware work order.  Workgroups are dealt round-robin over the 8 XCDs (observed, not contractual:
// b and b+8 share an XCD and its private 4 MiB L2), while the work list is pair-major (all candidate
// blocks of a pair are adjacent).  With the identity mapping every pair's point sets and tables are
// pulled into all eight L2s; this bijective remap hands each XCD one contiguous eighth of the list, so
// a pair is fetched from HBM by one XCD (or two, at a boundary).  Speed/traffic only, never correctness.
static __device__ __forceinline__ int xcd_work_index(int b, int n)
{
    const int q = n >> 3, r = n & 7, x = b & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
}

}  // namespace mm
