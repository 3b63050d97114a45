// mm_smooth_kernels.hip -- CCTA mesh finishing for gfx950: the sorted vertex adjacency (CSR), Laplacian / Taubin steps
// over it, ring distances from seed vertices and the largest displacement.
//
// trimesh.smoothing.filter_taubin / filter_laplacian (equal weights) as multimodars/ccta/fixing_functions.py:52-92 ends
// its post-processing, with the row order fixed: include/mm_ccta.h ("mesh smoothing") states the rules, every one of
// which has a single answer whatever the scheduling.
//
//   k_smooth_degree      one lane per slot of the edge table of mm_mesh_device.h (each undirected edge once): an edge
//                        between two different vertices adds one to the degree of both ends (integer atomics) and is
//                        counted, one atomicAdd per wave.
//   k_smooth_scan_count / k_smooth_scan_tiles / k_smooth_scan_offsets   the exclusive scan of the int32 degrees in the
//                        three passes of mm_mesh_device.h's scan (tiles of 4096): off[v], off[nv] = the entries; the degree
//                        array becomes the fill cursor in place.  The last pass also counts the isolated vertices and
//                        takes the largest degree (one integer atomic per wave each).
//   k_smooth_fill        every edge writes each end into the other's row through the atomic cursor: the order inside a
//                        row is whatever the scheduling made it ...
//   k_smooth_row_sort    ... and one lane per row sorts it ascending, in place: insertion for the short rows nearly all
//                        are, heap sort beyond (a fan centre's row is as long as its loop).  The sort is what makes the
//                        CSR deterministic.
//   k_smooth_step        one lane per vertex: the row's neighbours gathered in row order (one 24-byte read each from the
//                        interleaved xyz of the previous step), acc = acc + w * x_j unfused, x' = x + f * (acc - x);
//                        isolated and pinned vertices keep their bits.  A row is never split across lanes: the order of
//                        the sum is the rule.  No floating-point atomics.
//   k_smooth_ring_seed / k_smooth_ring   level-synchronous pull: a vertex without a ring takes r where a neighbour holds
//                        r - 1; the vertices reached are counted by ballot, one atomicAdd per wave.
//   k_smooth_disp        max over vertices of (dx dx + dy dy) + dz dz as an integer atomicMax on the bits of the
//                        non-negative double, one per wave.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mm_device.h"
#include "mm_mesh_device.h"

namespace mm {

static constexpr int kSmoothInsertion = 24;                                    // rows up to here: insertion sort

// counts[0] += the edges between different vertices.  cap is a multiple of kMeshThreads, as is the stride.
__global__ void __launch_bounds__(kMeshThreads)
k_smooth_degree(const unsigned long long* __restrict__ keys, unsigned long long cap, int32_t* __restrict__ deg,
                unsigned long long* __restrict__ counts)
{
    for (unsigned long long s = (unsigned long long)mesh_tid(); s < cap; s += (unsigned long long)mesh_stride()) {
        const unsigned long long k = keys[s];
        const int32_t lo = (int32_t)edge_lo(k), hi = (int32_t)edge_hi(k);
        const bool edge = k != kEdgeEmpty && lo != hi;
        if (edge) {
            atomicAdd(&deg[lo], 1);
            atomicAdd(&deg[hi], 1);
        }
        wave_count(edge, &counts[0]);
    }
}

// tile_sum[t] = the sum of the degrees of tile t; grid = the number of tiles
__global__ void __launch_bounds__(kMeshThreads)
k_smooth_scan_count(const int32_t* __restrict__ deg, long long n, long long* __restrict__ tile_sum)
{
    const long long i0 = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
    long long c = 0;
    for (int j = 0; j < kScanItems; ++j)
        if (i0 + j < n) c += deg[i0 + j];
    long long total;
    block_exclusive<kMeshThreads>(c, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// one workgroup: tile_sum -> exclusive offsets in place; off[n] = the total
__global__ void __launch_bounds__(kMeshThreads)
k_smooth_scan_tiles(long long* __restrict__ tile_sum, long long n_tiles, int32_t* __restrict__ off, long long n)
{
    const long long total = scan_tile_sums(tile_sum, n_tiles);
    if (threadIdx.x == 0) off[n] = (int32_t)total;
}

// off[i] = the sum of the degrees before i; deg[i] becomes the same (the fill cursor of row i); counts[1] += the
// vertices of degree 0, counts[2] = max(counts[2], the largest degree)
__global__ void __launch_bounds__(kMeshThreads)
k_smooth_scan_offsets(int32_t* __restrict__ deg, long long n, const long long* __restrict__ tile_off,
                      int32_t* __restrict__ off, unsigned long long* __restrict__ counts)
{
    const long long i0 = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
    int32_t d[kScanItems];
    long long c = 0;
    int isolated = 0;
    int32_t longest = 0;
    for (int j = 0; j < kScanItems; ++j) {
        d[j] = i0 + j < n ? deg[i0 + j] : -1;
        if (d[j] > 0) c += d[j];
        isolated += d[j] == 0;
        longest = d[j] > longest ? d[j] : longest;
    }
    long long total;
    long long at = tile_off[blockIdx.x] + block_exclusive<kMeshThreads>(c, &total);
    for (int j = 0; j < kScanItems; ++j) {
        if (d[j] >= 0) {
            off[i0 + j] = (int32_t)at;
            deg[i0 + j] = (int32_t)at;
            at += d[j];
        }
    }
    for (int s = 1; s < 64; s <<= 1) {
        isolated += __shfl_xor(isolated, s);
        const int32_t other = __shfl_xor(longest, s);
        longest = other > longest ? other : longest;
    }
    if (__lane_id() == 0) {
        if (isolated) atomicAdd(&counts[1], (unsigned long long)isolated);
        if (longest) atomicMax(&counts[2], (unsigned long long)longest);
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_smooth_fill(const unsigned long long* __restrict__ keys, unsigned long long cap, int32_t* __restrict__ cursor,
              int32_t* __restrict__ nb)
{
    for (unsigned long long s = (unsigned long long)mesh_tid(); s < cap; s += (unsigned long long)mesh_stride()) {
        const unsigned long long k = keys[s];
        const int32_t lo = (int32_t)edge_lo(k), hi = (int32_t)edge_hi(k);
        if (k == kEdgeEmpty || lo == hi) continue;
        nb[atomicAdd(&cursor[lo], 1)] = hi;
        nb[atomicAdd(&cursor[hi], 1)] = lo;
    }
}

static __device__ __forceinline__ void smooth_sift(int32_t* __restrict__ r, int32_t root, int32_t n)
{
    const int32_t x = r[root];
    for (;;) {
        int32_t c = 2 * root + 1;
        if (c >= n) break;
        if (c + 1 < n && r[c + 1] > r[c]) ++c;
        if (r[c] <= x) break;
        r[root] = r[c];
        root = c;
    }
    r[root] = x;
}

// row v of nb ascending, in place (the entries of a row are distinct)
__global__ void __launch_bounds__(kMeshThreads)
k_smooth_row_sort(const int32_t* __restrict__ off, int32_t* __restrict__ nb, long long nv)
{
    for (long long v = mesh_tid(); v < nv; v += mesh_stride()) {
        int32_t* r = nb + off[v];
        const int32_t n = off[v + 1] - off[v];
        if (n <= kSmoothInsertion) {
            for (int32_t i = 1; i < n; ++i) {
                const int32_t x = r[i];
                int32_t j = i;
                for (; j > 0 && r[j - 1] > x; --j) r[j] = r[j - 1];
                r[j] = x;
            }
            continue;
        }
        for (int32_t i = n / 2 - 1; i >= 0; --i) smooth_sift(r, i, n);
        for (int32_t m = n - 1; m > 0; --m) {
            const int32_t t = r[0];
            r[0] = r[m];
            r[m] = t;
            smooth_sift(r, 0, m);
        }
    }
}

// one step with factor f: out = the coordinates after it, in = those before (never the same buffer)
__global__ void __launch_bounds__(kMeshThreads)
k_smooth_step(const int32_t* __restrict__ off, const int32_t* __restrict__ nb, const double* __restrict__ in,
              double* __restrict__ out, long long nv, double f, const uint8_t* __restrict__ pinned)
{
    for (long long v = mesh_tid(); v < nv; v += mesh_stride()) {
        const int32_t b = off[v], e = off[v + 1];
        const double x = in[3 * v], y = in[3 * v + 1], z = in[3 * v + 2];
        double nx = x, ny = y, nz = z;
        if (e > b && !(pinned && pinned[v])) {
            const double w = 1.0 / (double)(e - b);
            double ax = 0.0, ay = 0.0, az = 0.0;
            for (int32_t k = b; k < e; ++k) {
                const double* p = in + 3 * (long long)nb[k];
                ax = ax + w * p[0];
                ay = ay + w * p[1];
                az = az + w * p[2];
            }
            nx = x + f * (ax - x);
            ny = y + f * (ay - y);
            nz = z + f * (az - z);
        }
        out[3 * v] = nx;
        out[3 * v + 1] = ny;
        out[3 * v + 2] = nz;
    }
}

// ring (all -1 before) = 0 at the seeds; *reached += the distinct seeds
__global__ void __launch_bounds__(kMeshThreads)
k_smooth_ring_seed(const int32_t* __restrict__ seeds, long long n_padded, long long n, int32_t* __restrict__ ring,
                   unsigned long long* __restrict__ reached)
{
    for (long long i = mesh_tid(); i < n_padded; i += mesh_stride()) {
        const bool first = i < n && atomicExch(&ring[seeds[i]], 0) == -1;
        wave_count(first, reached);
    }
}

// ring r (>= 1): a vertex holding -1 with a neighbour holding r - 1 takes r.  A neighbour written in this very launch
// reads as -1 or r, neither of which is r - 1.  *reached += the vertices set.
__global__ void __launch_bounds__(kMeshThreads)
k_smooth_ring(const int32_t* __restrict__ off, const int32_t* __restrict__ nb, long long nv_padded, long long nv,
              int32_t* __restrict__ ring, int32_t r, unsigned long long* __restrict__ reached)
{
    for (long long v = mesh_tid(); v < nv_padded; v += mesh_stride()) {
        bool take = false;
        if (v < nv && __atomic_load_n(&ring[v], __ATOMIC_RELAXED) == -1) {
            for (int32_t k = off[v], e = off[v + 1]; k < e && !take; ++k)
                take = __atomic_load_n(&ring[nb[k]], __ATOMIC_RELAXED) == r - 1;
            if (take) __atomic_store_n(&ring[v], r, __ATOMIC_RELAXED);
        }
        wave_count(take, reached);
    }
}

// *max_bits = max(*max_bits, the bits of (dx dx + dy dy) + dz dz) over the vertices, d = b - a
__global__ void __launch_bounds__(kMeshThreads)
k_smooth_disp(const double* __restrict__ a, const double* __restrict__ b, long long nv,
              unsigned long long* __restrict__ max_bits)
{
    unsigned long long m = 0;
    for (long long v = mesh_tid(); v < nv; v += mesh_stride()) {
        const double dx = b[3 * v] - a[3 * v], dy = b[3 * v + 1] - a[3 * v + 1], dz = b[3 * v + 2] - a[3 * v + 2];
        const unsigned long long q = (unsigned long long)__double_as_longlong((dx * dx + dy * dy) + dz * dz);
        m = q > m ? q : m;
    }
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned long long other = (unsigned long long)__shfl_xor((long long)m, s);
        m = other > m ? other : m;
    }
    if (__lane_id() == 0 && m) atomicMax(max_bits, m);
}

// every launcher here counts the kernels it launched
#define SMOOTH_LAUNCH(kernel, blocks, ...) do { MESH_LAUNCH(kernel, blocks, __VA_ARGS__); ++*launches; } while (0)

size_t mesh_csr_tiles(long long nv) { return scan_tiles(nv); }

hipError_t launch_mesh_row_offsets(int32_t* deg, long long n, int32_t* off, long long* tile_sum, unsigned long long* counts,
                                   int* launches, hipStream_t s)
{
    const long long tiles = (long long)scan_tiles(n);
    SMOOTH_LAUNCH(k_smooth_scan_count, (unsigned)tiles, deg, n, tile_sum);
    SMOOTH_LAUNCH(k_smooth_scan_tiles, 1u, tile_sum, tiles, off, n);
    SMOOTH_LAUNCH(k_smooth_scan_offsets, (unsigned)tiles, deg, n, tile_sum, off, counts);
    return hipSuccess;
}

hipError_t launch_mesh_row_sort(const int32_t* off, int32_t* nb, long long n, int* launches, hipStream_t s)
{
    SMOOTH_LAUNCH(k_smooth_row_sort, mesh_grid(n), off, nb, n);
    return hipSuccess;
}

hipError_t launch_mesh_csr(const unsigned long long* keys, int log2_cap, long long nv, int32_t* deg, int32_t* off,
                           long long* tile_sum, int32_t* nb, unsigned long long* counts, int* launches, hipStream_t s)
{
    const unsigned long long cap = 1ull << log2_cap;                   // at least kMeshThreads (the host sizes it)
    hipError_t he;
    if ((he = hipMemsetAsync(deg, 0, (size_t)nv * 4, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(counts, 0, 4 * 8, s)) != hipSuccess) return he;
    SMOOTH_LAUNCH(k_smooth_degree, mesh_grid((long long)cap), keys, cap, deg, counts);
    if ((he = launch_mesh_row_offsets(deg, nv, off, tile_sum, counts, launches, s)) != hipSuccess) return he;
    SMOOTH_LAUNCH(k_smooth_fill, mesh_grid((long long)cap), keys, cap, deg, nb);
    return launch_mesh_row_sort(off, nb, nv, launches, s);
}

hipError_t launch_mesh_step(const int32_t* off, const int32_t* nb, const double* in, double* out, long long nv, double f,
                            const uint8_t* pinned, int* launches, hipStream_t s)
{
    SMOOTH_LAUNCH(k_smooth_step, mesh_grid(nv), off, nb, in, out, nv, f, pinned);
    return hipSuccess;
}

hipError_t launch_mesh_ring_seed(const int32_t* seeds, long long n, int32_t* ring, long long nv,
                                 unsigned long long* reached, int* launches, hipStream_t s)
{
    hipError_t he;
    if ((he = hipMemsetAsync(ring, 0xFF, (size_t)nv * 4, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(reached, 0, 8, s)) != hipSuccess) return he;
    if (n > 0) SMOOTH_LAUNCH(k_smooth_ring_seed, mesh_grid(n), seeds, mesh_pad(n), n, ring, reached);
    return hipSuccess;
}

hipError_t launch_mesh_ring(const int32_t* off, const int32_t* nb, long long nv, int32_t* ring, int32_t r,
                            unsigned long long* reached, int* launches, hipStream_t s)
{
    SMOOTH_LAUNCH(k_smooth_ring, mesh_grid(nv), off, nb, mesh_pad(nv), nv, ring, r, reached);
    return hipSuccess;
}

hipError_t launch_mesh_disp(const double* a, const double* b, long long nv, unsigned long long* max_bits, int* launches,
                            hipStream_t s)
{
    const hipError_t he = hipMemsetAsync(max_bits, 0, 8, s);
    if (he != hipSuccess) return he;
    SMOOTH_LAUNCH(k_smooth_disp, mesh_grid(nv), a, b, nv, max_bits);
    return hipSuccess;
}

}  // namespace mm
