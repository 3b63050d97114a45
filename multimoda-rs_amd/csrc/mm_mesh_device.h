// mm_mesh_device.h -- what the CCTA mesh kernel files (mm_trim, mm_weld, mm_close, mm_smooth, mm_rim, mm_refine, mm_relax,
// mm_flip, mm_collapse, mm_repair, mm_geodesic, mm_clip _kernels.hip) share, the device-side counterpart of mm_stage.h: the launch geometry, the 64-bit edge table (the weld, trim, refine, flip, collapse and repair files
// insert, the close, smooth, flip, collapse and geodesic files read, EdgeTable of mm_stage.h sizes it) with the insert
// kernel and the clear the flips and the collapse share, the first-index-wins table and the hooking union-find of the
// weld, the repair and the clip, the workgroup scan and the two per-wave ballot idioms.  Header-only; internal.
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
// f << 1 | (f traverses the edge from the smaller to the larger end).  Returns the slot.
template <bool kOwners>
static __device__ __forceinline__ unsigned long long edge_insert(unsigned long long* __restrict__ keys, unsigned int* __restrict__ cnt,
                                                   unsigned int* __restrict__ own, unsigned long long mask, int shift,
                                                   int32_t u, int32_t v, unsigned int f)
{
    const unsigned long long s = edge_claim(keys, mask, shift, u, v);
    const unsigned int p = atomicAdd(&cnt[s], 1u);
    if (kOwners && p < 2) own[2 * s + p] = (f << 1) | (u < v ? 1u : 0u);
    return s;
}

// The table of the flips and the collapse: owners, and per slot in `first` the smallest corner id (3 f + the corner the
// edge starts at) of the faces that own it -- what makes a priority unique.  One lane per face; kLive: only the faces
// with fkeep set.
template <bool kLive>
__global__ void __launch_bounds__(kMeshThreads)
k_edge_insert_first(const int32_t* __restrict__ face, long long nf, const uint8_t* __restrict__ fkeep,
                    unsigned long long* __restrict__ keys, unsigned int* __restrict__ cnt, unsigned int* __restrict__ own,
                    unsigned int* __restrict__ first, unsigned long long mask, int shift)
{
    for (long long f = mesh_tid(); f < nf; f += mesh_stride()) {
        if (kLive && !fkeep[f]) continue;
        int32_t c[3] = {face[3 * f], face[3 * f + 1], face[3 * f + 2]};
        for (int j = 0; j < 3; ++j) {
            const unsigned long long s = edge_insert<true>(keys, cnt, own, mask, shift, c[j], c[j == 2 ? 0 : j + 1], (unsigned int)f);
            atomicMin(&first[s], (unsigned int)(3 * f + j));
        }
    }
}

// that table and the words beside it before an insertion: keys, cnt and first of cap slots, the nv vertex words, the
// first n_counts counters
inline hipError_t edge_first_clear(unsigned long long* keys, unsigned int* cnt, unsigned int* first, unsigned long long cap,
                                   unsigned int* vw, long long nv, unsigned long long* counts, int n_counts, hipStream_t s)
{
    hipError_t he;
    if ((he = hipMemsetAsync(keys, 0xFF, cap * 8, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(cnt, 0, cap * 4, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(first, 0xFF, cap * 4, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(vw, 0, (size_t)nv * 4, s)) != hipSuccess) return he;
    return hipMemsetAsync(counts, 0, (size_t)n_counts * 8, s);
}

// ---- the first-index-wins table (the welds of mm_weld_kernels.hip, the repair's duplicates): open addressing over int32
// slots, kFirstEmpty before, each ending as the SMALLEST index inserted with the slot's key.  A slot is claimed with a
// 32-bit atomicCAS from empty; a lane that finds it taken asks same(holder) -- every holder of a slot has one key, so
// whichever it reads answers, provided the key derives from memory no lane writes -- and lowers the slot with atomicMin
// or probes on.  Returns the slot of i's key; its final value is read in a later launch. ----

static constexpr int32_t kFirstEmpty = -1;

static __device__ __forceinline__ unsigned long long mesh_mix(unsigned long long h, unsigned long long k)
{
    h ^= k + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
    h *= 0xBF58476D1CE4E5B9ull;
    return h ^ (h >> 31);
}

template <class Same>
static __device__ __forceinline__ int32_t first_index_insert(int32_t* __restrict__ table, unsigned long long mask,
                                                             unsigned long long s, int32_t i, Same same)
{
    for (;;) {
        const int32_t o = atomicCAS(&table[s], kFirstEmpty, i);
        if (o != kFirstEmpty) {
            if (!same(o)) { s = (s + 1) & mask; continue; }
            if (i < o) atomicMin(&table[s], i);
        }
        return (int32_t)s;
    }
}

static __device__ __forceinline__ void mesh_sort3(int32_t a, int32_t b, int32_t c, int32_t k[3])
{
    int32_t t;
    if (a > b) { t = a; a = b; b = t; }
    if (b > c) { t = b; b = c; c = t; }
    if (a > b) { t = a; a = b; b = t; }
    k[0] = a; k[1] = b; k[2] = c;
}

// where the probe of a sorted index triple starts
static __device__ __forceinline__ unsigned long long mesh_triple_slot(const int32_t k[3], int shift)
{
    return mesh_mix(mesh_mix(0, ((unsigned long long)k[0] << 32) | (unsigned long long)k[1]), (unsigned long long)k[2]) >> shift;
}

// ---- the hooking union-find (the winding of mm_weld_kernels.hip over faces, the repair over corners): link[x] =
// parent << 1 | parity to the parent, x << 1 at a root.  A root hooks under a smaller root with one atomicCAS (parents
// only ever get smaller: no cycle, and the root of a set ends as its smallest member, whatever the order of arrival);
// finds halve their path as they go.  Lock-free: a lane only retries after another lane's hook landed.  Rounds of
// k_weld_jump flatten the links afterwards. ----

static __device__ __forceinline__ unsigned int uf_load(const unsigned int* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// the root of x and, xor-ed into *par, x's parity to it; every step moves x's link to its grandparent (any ancestor with
// the parities added is a valid link, whichever lane writes it last)
static __device__ __forceinline__ unsigned int uf_find(unsigned int* __restrict__ link, unsigned int x, unsigned int* par)
{
    unsigned int wx = uf_load(&link[x]);
    while ((wx >> 1) != x) {
        const unsigned int p = wx >> 1;
        const unsigned int wp = uf_load(&link[p]);
        if ((wp >> 1) != p) __atomic_store_n(&link[x], (wp & ~1u) | ((wx ^ wp) & 1u), __ATOMIC_RELAXED);
        *par ^= wx & 1u;
        x = p;
        wx = wp;
    }
    return x;
}

// the sets of a and b become one, with parity e between a and b (0 where parities are not in use)
static __device__ __forceinline__ void uf_union(unsigned int* __restrict__ link, unsigned int a, unsigned int b, unsigned int e)
{
    unsigned int pa = 0, pb = 0;
    for (;;) {
        a = uf_find(link, a, &pa);
        b = uf_find(link, b, &pb);
        if (a == b) break;                                          // joined already (or not orientable)
        const unsigned int hi = a < b ? b : a, lo = a < b ? a : b;
        if (atomicCAS(&link[hi], hi << 1, (lo << 1) | (pa ^ pb ^ e)) == hi << 1) break;
    }
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
