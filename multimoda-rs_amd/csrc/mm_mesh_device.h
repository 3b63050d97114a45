// mm_mesh_device.h -- what the CCTA mesh kernel files (mm_trim, mm_weld, mm_close, mm_smooth, mm_rim, mm_refine, mm_flip,
// mm_collapse _kernels.hip) share, the device-side counterpart of mm_stage.h: the launch geometry, the 64-bit edge table (the weld, trim,
// refine and flip files insert, the close, smooth and flip files read, EdgeTable of mm_stage.h sizes it), the workgroup scan
// and the two per-wave ballot idioms.  Header-only; internal.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace mm {

static constexpr int kMeshThreads = 256;
static constexpr int kScanItems = 16;                                  // items per lane in a scan
static constexpr int kScanTile = kMeshThreads * kScanItems;            // 4096 per workgroup
static constexpr unsigned long long kEdgeEmpty = ~0ull;                // no key: both ends < 2^31 never give it

static __device__ __forceinline__ long long mesh_tid() { return (long long)blockIdx.x * blockDim.x + threadIdx.x; }
static __device__ __forceinline__ long long mesh_stride() { return (long long)gridDim.x * blockDim.x; }

// one lane per item in a grid-stride loop: the workgroups of n items, at least one and at most 65536
inline unsigned mesh_grid(long long n)
{
    const long long b = (n + kMeshThreads - 1) / kMeshThreads;
    return (unsigned)(b < 1 ? 1 : (b > 65536 ? 65536 : b));
}

// n up to a multiple of the workgroup: the trip count of a loop whose every wave has to stay whole (the ballots)
inline long long mesh_pad(long long n) { return (n + kMeshThreads - 1) / kMeshThreads * kMeshThreads; }

inline size_t scan_tiles(long long n) { return (size_t)((n + kScanTile - 1) / kScanTile); }

// on the stream `s` of the enclosing launcher, which returns the error of a launch that failed
#define MESH_LAUNCH(kernel, blocks, ...)                                                                   \
    do {                                                                                                   \
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kMeshThreads), 0, s, __VA_ARGS__);                   \
        const hipError_t he__ = hipGetLastError();                                                         \
        if (he__ != hipSuccess) return he__;                                                               \
    } while (0)

// ---- the edge table: cap = mask + 1 slots (a power of two, at least twice the insertions, so a probe ends), open
// addressing with linear probing; a slot is a 64-bit key (kEdgeEmpty before), a 32-bit count and, where the table has
// them, the first two owners ----

// the undirected edge u - v: min << 32 | max
static __device__ __forceinline__ unsigned long long edge_key(int32_t u, int32_t v)
{
    const unsigned long long lo = (unsigned long long)(u < v ? u : v), hi = (unsigned long long)(u < v ? v : u);
    return (lo << 32) | hi;
}

// where the probe of a key starts: its multiplicative hash >> shift (64 - log2 cap)
static __device__ __forceinline__ unsigned long long edge_slot(unsigned long long key, int shift)
{
    return (key * 0x9E3779B97F4A7C15ull) >> shift;
}

static __device__ __forceinline__ unsigned int edge_lo(unsigned long long key) { return (unsigned int)(key >> 32); }
static __device__ __forceinline__ unsigned int edge_hi(unsigned long long key) { return (unsigned int)(key & 0xFFFFFFFFull); }

// the slot of the undirected edge u - v, taken with a 64-bit atomicCAS on the key where no lane held it yet
static __device__ __forceinline__ unsigned long long edge_claim(unsigned long long* __restrict__ keys,
                                                                unsigned long long mask, int shift, int32_t u, int32_t v)
{
    const unsigned long long key = edge_key(u, v);
    unsigned long long s = edge_slot(key, shift);
    for (;;) {
        const unsigned long long prev = atomicCAS(&keys[s], kEdgeEmpty, key);
        if (prev == kEdgeEmpty || prev == key) return s;
        s = (s + 1) & mask;
    }
}

// the slot of the undirected edge u - v in a table nothing inserts into any more, kEdgeEmpty where it has none
static __device__ __forceinline__ unsigned long long edge_find(const unsigned long long* __restrict__ keys,
                                                               unsigned long long mask, int shift, int32_t u, int32_t v)
{
    const unsigned long long key = edge_key(u, v);
    unsigned long long s = edge_slot(key, shift);
    for (;;) {
        const unsigned long long at = keys[s];
        if (at == key) return s;
        if (at == kEdgeEmpty) return kEdgeEmpty;
        s = (s + 1) & mask;
    }
}

// the edge u - v of face f: its slot claimed, 32-bit atomicAdd on its count; with owners, the first two to arrive leave
// f << 1 | (f traverses the edge from the smaller to the larger end)
template <bool kOwners>
static __device__ __forceinline__ void edge_insert(unsigned long long* __restrict__ keys, unsigned int* __restrict__ cnt,
                                                   unsigned int* __restrict__ own, unsigned long long mask, int shift,
                                                   int32_t u, int32_t v, unsigned int f)
{
    const unsigned long long s = edge_claim(keys, mask, shift, u, v);
    const unsigned int p = atomicAdd(&cnt[s], 1u);
    if (kOwners && p < 2) own[2 * s + p] = (f << 1) | (u < v ? 1u : 0u);
}

// ---- scans ----

// inclusive sum over the workgroup of one value per lane; returns the lane's exclusive prefix, *total the sum
template <int kThreads>
static __device__ __forceinline__ long long block_exclusive(long long x, long long* total)
{
    __shared__ long long s_wave[kThreads / 64];
    const int lane = (int)__lane_id(), wave = threadIdx.x >> 6;
    long long inc = x;
    for (int d = 1; d < 64; d <<= 1) {
        const long long y = __shfl_up(inc, d);
        if (lane >= d) inc += y;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    long long before = 0, all = 0;
    for (int w = 0; w < kThreads / 64; ++w) {
        const long long t = s_wave[w];
        if (w < wave) before += t;
        all += t;
    }
    __syncthreads();
    *total = all;
    return before + inc - x;
}

// one workgroup: the per-tile sums of a three-pass scan (tile sums, this, per-element offsets) -> exclusive offsets in
// place, kMeshThreads tiles a round with the carry of the rounds before; returns the total
static __device__ __forceinline__ long long scan_tile_sums(long long* tile_sum, long long n_tiles)
{
    long long carry = 0;
    for (long long t0 = 0; t0 < n_tiles; t0 += kMeshThreads) {
        const long long t = t0 + threadIdx.x;
        const long long x = t < n_tiles ? tile_sum[t] : 0;
        long long total;
        const long long ex = block_exclusive<kMeshThreads>(x, &total);
        if (t < n_tiles) tile_sum[t] = carry + ex;
        carry += total;
    }
    return carry;
}

// ---- ballots: every lane of the wave has to arrive (loops over mesh_pad(n) or a table's cap) ----

// *counter += the lanes of the wave with pred: lane 0 adds the ballot's popcount
static __device__ __forceinline__ void wave_count(bool pred, unsigned long long* counter)
{
    const int lane = (int)__lane_id();
    const unsigned long long b = __ballot(pred);
    if (lane == 0 && b) atomicAdd(counter, (unsigned long long)__popcll(b));
}

// the wave takes room for its lanes with pred through one returning atomicAdd; returns the lane's slot (its rank in the
// ballot after the wave's base), meaningful where pred
static __device__ __forceinline__ unsigned long long wave_append(bool pred, unsigned long long* n_out)
{
    const int lane = (int)__lane_id();
    const unsigned long long below = (1ull << lane) - 1;                 // the lanes before this one
    const unsigned long long b = __ballot(pred);
    unsigned long long base = 0;
    if (lane == 0 && b) base = atomicAdd(n_out, (unsigned long long)__popcll(b));
    base = __shfl(base, 0);
    return base + (unsigned long long)__popcll(b & below);
}

}  // namespace mm
