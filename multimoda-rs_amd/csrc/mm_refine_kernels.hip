// mm_refine_kernels.hip -- CCTA mesh refinement for gfx950: long edges split at their midpoint, pass after pass, until
// none is longer than the threshold.
//
// The edge split of an isotropic remesh (multimodars/ccta/fixing_functions.py:114-239 hands the whole remesh to MeshLab;
// the flip is mm_flip_kernels.hip, relaxation and reprojection mm_relax_kernels.hip, the collapse
// mm_collapse_kernels.hip).  include/mm_ccta.h ("mesh refinement")
// states the rule, which has one answer whatever the scheduling: a marked edge's vertex number follows the smallest
// corner id 3 f + j that names the edge, found with an integer atomicMin.  One lane per item in grid-stride loops (the
// scan kernels: one workgroup per tile of mm_mesh_device.h's scan); integer atomics only.
//
//   k_refine_edge_insert  the three edges of every face into the edge table of mm_mesh_device.h: a count, the smallest
//                         corner id (own[2 s]) and, per corner, the slot it landed in, so that nothing probes twice.
//   k_refine_mark         one lane per slot: own[2 s + 1] = 0 for a marked edge, ~0 otherwise; the edges between
//                         different vertices, the open and the non-manifold ones and the marked ones are counted by
//                         ballot, the longest squared length is an integer atomicMax on the bits, one per wave.
//   k_refine_count        per face a code (bits 0-2: the corner's edge is marked, bits 3-5: and this corner is its first)
//                         and, packed in one 64-bit sum, the new vertices (low half) and children (high half) of the
//                         tile; the faces with 1, 2, 3 marked corners are counted, one atomicAdd per wave each.
//   k_refine_scan_tiles   one workgroup: the tile sums -> exclusive offsets, the totals into the counters.
//   k_refine_offsets      the scan's third pass: the first child of every face; every first corner writes its edge's
//                         vertex number into own[2 s + 1], the midpoint and the parents (or, for the edge list, the edge
//                         and its squared length).
//   k_refine_children     every face writes its 1 .. 4 children.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mm_device.h"
#include "mm_mesh_device.h"

namespace mm {

static constexpr unsigned int kRefineUnmarked = ~0u;
enum { kRefEdges = 0, kRefOpen, kRefNonManifold, kRefLongest, kRefMarked, kRefOne, kRefTwo, kRefThree, kRefNewVerts,
       kRefChildren, kRefCounters };

// ((dx dx + dy dy) + dz dz) of d = q - p, unfused
static __device__ __forceinline__ double refine_len_sq(const double* __restrict__ p, const double* __restrict__ q)
{
    const double dx = q[0] - p[0], dy = q[1] - p[1], dz = q[2] - p[2];
    return (dx * dx + dy * dy) + dz * dz;
}

// the new vertices (low half) and the children (high half) of a face with this code
static __device__ __forceinline__ long long refine_packed(unsigned int code)
{
    return (long long)__popc(code >> 3) | ((long long)(1 + __popc(code & 7u)) << 32);
}

__global__ void __launch_bounds__(kMeshThreads)
k_refine_edge_insert(const int32_t* __restrict__ face, long long nf, unsigned long long* __restrict__ keys,
                     unsigned int* __restrict__ cnt, unsigned int* __restrict__ own, unsigned long long mask, int shift,
                     unsigned int* __restrict__ slot)
{
    for (long long f = mesh_tid(); f < nf; f += mesh_stride()) {
        const int32_t a = face[3 * f], b = face[3 * f + 1], c = face[3 * f + 2];
        const unsigned int id = (unsigned int)(3 * f);
        const unsigned long long s0 = edge_claim(keys, mask, shift, a, b);
        const unsigned long long s1 = edge_claim(keys, mask, shift, b, c);
        const unsigned long long s2 = edge_claim(keys, mask, shift, c, a);
        atomicAdd(&cnt[s0], 1u);
        atomicAdd(&cnt[s1], 1u);
        atomicAdd(&cnt[s2], 1u);
        atomicMin(&own[2 * s0], id);
        atomicMin(&own[2 * s1], id + 1);
        atomicMin(&own[2 * s2], id + 2);
        slot[3 * f] = (unsigned int)s0;
        slot[3 * f + 1] = (unsigned int)s1;
        slot[3 * f + 2] = (unsigned int)s2;
    }
}

// cap is a multiple of kMeshThreads, as is the stride.  all != 0: every edge between different vertices is marked.
__global__ void __launch_bounds__(kMeshThreads)
k_refine_mark(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ cnt,
              unsigned int* __restrict__ own, unsigned long long cap, const double* __restrict__ v, double thr2, int all,
              unsigned long long* __restrict__ counts)
{
    for (unsigned long long s = (unsigned long long)mesh_tid(); s < cap; s += (unsigned long long)mesh_stride()) {
        const unsigned long long k = keys[s];
        const bool used = k != kEdgeEmpty;
        const unsigned int lo = edge_lo(k), hi = edge_hi(k);
        const bool edge = used && lo != hi;
        const unsigned int c = used ? cnt[s] : 0u;
        double d2 = 0.0;
        if (edge) d2 = refine_len_sq(v + 3 * (long long)lo, v + 3 * (long long)hi);
        const bool marked = edge && (all != 0 || d2 > thr2);
        if (used) own[2 * s + 1] = marked ? 0u : kRefineUnmarked;
        unsigned long long m = edge && d2 == d2 ? (unsigned long long)__double_as_longlong(d2) : 0ull;
        for (int x = 1; x < 64; x <<= 1) {
            const unsigned long long other = (unsigned long long)__shfl_xor((long long)m, x);
            m = other > m ? other : m;
        }
        if (__lane_id() == 0 && m) atomicMax(&counts[kRefLongest], m);
        wave_count(edge, &counts[kRefEdges]);
        wave_count(c == 1u, &counts[kRefOpen]);
        wave_count(c > 2u, &counts[kRefNonManifold]);
        wave_count(marked, &counts[kRefMarked]);
    }
}

// the code of face f
static __device__ __forceinline__ unsigned int refine_code(const unsigned int* __restrict__ slot,
                                                           const unsigned int* __restrict__ own, long long f)
{
    unsigned int code = 0;
    for (int j = 0; j < 3; ++j) {
        const unsigned long long s = slot[3 * f + j];
        const bool marked = own[2 * s + 1] != kRefineUnmarked;
        const bool first = own[2 * s] == (unsigned int)(3 * f + j);
        code |= (marked ? 1u : 0u) << j;
        code |= (marked && first ? 1u : 0u) << (3 + j);
    }
    return code;
}

// grid = the number of tiles
__global__ void __launch_bounds__(kMeshThreads)
k_refine_count(const unsigned int* __restrict__ slot, const unsigned int* __restrict__ own, long long nf,
               uint8_t* __restrict__ code, long long* __restrict__ tile_sum, unsigned long long* __restrict__ counts)
{
    const long long i0 = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
    long long c = 0;
    int one = 0, two = 0, three = 0;
    for (int j = 0; j < kScanItems; ++j) {
        const long long f = i0 + j;
        if (f >= nf) break;
        const unsigned int x = refine_code(slot, own, f);
        code[f] = (uint8_t)x;
        c += refine_packed(x);
        const int n = __popc(x & 7u);
        one += n == 1;
        two += n == 2;
        three += n == 3;
    }
    long long total;
    block_exclusive<kMeshThreads>(c, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
    for (int x = 1; x < 64; x <<= 1) {
        one += __shfl_xor(one, x);
        two += __shfl_xor(two, x);
        three += __shfl_xor(three, x);
    }
    if (__lane_id() == 0) {
        if (one) atomicAdd(&counts[kRefOne], (unsigned long long)one);
        if (two) atomicAdd(&counts[kRefTwo], (unsigned long long)two);
        if (three) atomicAdd(&counts[kRefThree], (unsigned long long)three);
    }
}

// one workgroup
__global__ void __launch_bounds__(kMeshThreads)
k_refine_scan_tiles(long long* __restrict__ tile_sum, long long n_tiles, unsigned long long* __restrict__ counts)
{
    const long long total = scan_tile_sums(tile_sum, n_tiles);
    if (threadIdx.x == 0) {
        counts[kRefNewVerts] = (unsigned long long)(total & 0xFFFFFFFFll);
        counts[kRefChildren] = (unsigned long long)(total >> 32);
    }
}

// grid = the number of tiles.  foff[f] = the first child of face f.  The k-th first corner (k counted from base) takes
// the number base + k: with kList the edge and its squared length go to edges / len_sq at k; without, own[2 s + 1] =
// base + k, the midpoint goes to v_out at base + k and the parents to par at base + k - par_base.
template <bool kList>
__global__ void __launch_bounds__(kMeshThreads)
k_refine_offsets(const uint8_t* __restrict__ code, long long nf, const long long* __restrict__ tile_off,
                 const unsigned int* __restrict__ slot, const unsigned long long* __restrict__ keys,
                 unsigned int* __restrict__ own, const double* __restrict__ v, long long base, long long par_base,
                 int32_t* __restrict__ foff, double* __restrict__ v_out, int32_t* __restrict__ par,
                 int32_t* __restrict__ edges, double* __restrict__ len_sq)
{
    const long long i0 = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
    uint8_t x[kScanItems];
    long long c = 0;
    for (int j = 0; j < kScanItems; ++j) {
        x[j] = i0 + j < nf ? code[i0 + j] : (uint8_t)0xFF;
        if (x[j] != 0xFF) c += refine_packed(x[j]);
    }
    long long total;
    long long at = tile_off[blockIdx.x] + block_exclusive<kMeshThreads>(c, &total);
    for (int j = 0; j < kScanItems; ++j) {
        if (x[j] == 0xFF) continue;
        const long long f = i0 + j;
        if (!kList) foff[f] = (int32_t)(at >> 32);
        long long k = at & 0xFFFFFFFFll;
        for (int q = 0; q < 3; ++q) {
            if (!((x[j] >> (3 + q)) & 1u)) continue;
            const unsigned long long s = slot[3 * f + q];
            const unsigned long long key = keys[s];
            const int32_t lo = (int32_t)edge_lo(key), hi = (int32_t)edge_hi(key);
            const double* p = v + 3 * (long long)lo;
            const double* r = v + 3 * (long long)hi;
            if (kList) {
                edges[2 * k] = lo;
                edges[2 * k + 1] = hi;
                len_sq[k] = refine_len_sq(p, r);
            } else {
                const long long id = base + k;
                own[2 * s + 1] = (unsigned int)id;
                v_out[3 * id] = (p[0] + r[0]) * 0.5;
                v_out[3 * id + 1] = (p[1] + r[1]) * 0.5;
                v_out[3 * id + 2] = (p[2] + r[2]) * 0.5;
                par[2 * (id - par_base)] = lo;
                par[2 * (id - par_base) + 1] = hi;
            }
            ++k;
        }
        at += refine_packed(x[j]);
    }
}

static __device__ __forceinline__ void refine_put(int32_t* __restrict__ o, int32_t a, int32_t b, int32_t c)
{
    o[0] = a;
    o[1] = b;
    o[2] = c;
}

// v: the coordinates after the pass (the midpoints are there)
__global__ void __launch_bounds__(kMeshThreads)
k_refine_children(const int32_t* __restrict__ face, long long nf, const uint8_t* __restrict__ code,
                  const int32_t* __restrict__ foff, const unsigned int* __restrict__ slot,
                  const unsigned int* __restrict__ own, const double* __restrict__ v, int32_t* __restrict__ out)
{
    for (long long f = mesh_tid(); f < nf; f += mesh_stride()) {
        const int32_t c0 = face[3 * f], c1 = face[3 * f + 1], c2 = face[3 * f + 2];
        const unsigned int m = code[f] & 7u;
        int32_t* o = out + 3 * (long long)foff[f];
        if (m == 0) {
            refine_put(o, c0, c1, c2);
            continue;
        }
        const int32_t n0 = (m & 1u) ? (int32_t)own[2 * (unsigned long long)slot[3 * f] + 1] : -1;
        const int32_t n1 = (m & 2u) ? (int32_t)own[2 * (unsigned long long)slot[3 * f + 1] + 1] : -1;
        const int32_t n2 = (m & 4u) ? (int32_t)own[2 * (unsigned long long)slot[3 * f + 2] + 1] : -1;
        const int n = __popc(m);
        // the corner the rotated face starts at: the marked edge (one), behind the unmarked edge (two), 0 (three)
        int r = 0;
        if (n == 1) r = m == 1u ? 0 : (m == 2u ? 1 : 2);
        if (n == 2) r = m == 6u ? 1 : (m == 5u ? 2 : 0);                // unmarked corner 0, 1, 2 -> start 1, 2, 0
        const int32_t a = r == 0 ? c0 : (r == 1 ? c1 : c2);
        const int32_t b = r == 0 ? c1 : (r == 1 ? c2 : c0);
        const int32_t c = r == 0 ? c2 : (r == 1 ? c0 : c1);
        const int32_t m0 = r == 0 ? n0 : (r == 1 ? n1 : n2);
        const int32_t m1 = r == 0 ? n1 : (r == 1 ? n2 : n0);
        const int32_t m2 = r == 0 ? n2 : (r == 1 ? n0 : n1);
        if (n == 1) {
            refine_put(o, a, m0, c);
            refine_put(o + 3, m0, b, c);
        } else if (n == 2) {
            refine_put(o, m0, b, m1);
            const double d_m0c = refine_len_sq(v + 3 * (long long)m0, v + 3 * (long long)c);
            const double d_am1 = refine_len_sq(v + 3 * (long long)a, v + 3 * (long long)m1);
            if (d_m0c < d_am1) {
                refine_put(o + 3, a, m0, c);
                refine_put(o + 6, m0, m1, c);
            } else {
                refine_put(o + 3, a, m0, m1);
                refine_put(o + 6, a, m1, c);
            }
        } else {
            refine_put(o, a, m0, m2);
            refine_put(o + 3, m0, b, m1);
            refine_put(o + 6, m2, m1, c);
            refine_put(o + 9, m0, m1, m2);
        }
    }
}

size_t refine_tiles(long long nf) { return scan_tiles(nf); }
int    refine_counters() { return kRefCounters; }

hipError_t launch_refine_edges(const int32_t* face, long long nf, unsigned long long* keys, unsigned int* cnt,
                               unsigned int* own, int log2_cap, unsigned int* slot, hipStream_t s)
{
    const unsigned long long cap = 1ull << log2_cap;
    hipError_t he;
    if ((he = hipMemsetAsync(keys, 0xFF, cap * 8, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(cnt, 0, cap * 4, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(own, 0xFF, cap * 8, s)) != hipSuccess) return he;
    MESH_LAUNCH(k_refine_edge_insert, mesh_grid(nf), face, nf, keys, cnt, own, cap - 1, 64 - log2_cap, slot);
    return hipSuccess;
}

hipError_t launch_refine_marks(const unsigned long long* keys, const unsigned int* cnt, unsigned int* own, int log2_cap,
                               const double* v, double thr2, int all, unsigned long long* counts, hipStream_t s)
{
    const unsigned long long cap = 1ull << log2_cap;                   // at least kMeshThreads (the host sizes it)
    const hipError_t he = hipMemsetAsync(counts, 0, kRefCounters * 8, s);
    if (he != hipSuccess) return he;
    MESH_LAUNCH(k_refine_mark, mesh_grid((long long)cap), keys, cnt, own, cap, v, thr2, all, counts);
    return hipSuccess;
}

hipError_t launch_refine_counts(const unsigned int* slot, const unsigned int* own, long long nf, uint8_t* code,
                                long long* tile_sum, unsigned long long* counts, hipStream_t s)
{
    const long long tiles = (long long)scan_tiles(nf);
    MESH_LAUNCH(k_refine_count, (unsigned)tiles, slot, own, nf, code, tile_sum, counts);
    MESH_LAUNCH(k_refine_scan_tiles, 1u, tile_sum, tiles, counts);
    return hipSuccess;
}

hipError_t launch_refine_offsets(const uint8_t* code, long long nf, const long long* tile_off, const unsigned int* slot,
                                 const unsigned long long* keys, unsigned int* own, const double* v, long long nv,
                                 long long nv0, int32_t* foff, double* v_out, int32_t* par, hipStream_t s)
{
    MESH_LAUNCH(k_refine_offsets<false>, (unsigned)scan_tiles(nf), code, nf, tile_off, slot, keys, own, v, nv, nv0, foff,
                v_out, par, (int32_t*)nullptr, (double*)nullptr);
    return hipSuccess;
}

hipError_t launch_refine_edge_list(const uint8_t* code, long long nf, const long long* tile_off, const unsigned int* slot,
                                   const unsigned long long* keys, const double* v, int32_t* edges, double* len_sq,
                                   hipStream_t s)
{
    MESH_LAUNCH(k_refine_offsets<true>, (unsigned)scan_tiles(nf), code, nf, tile_off, slot, keys, (unsigned int*)nullptr, v,
                0ll, 0ll, (int32_t*)nullptr, (double*)nullptr, (int32_t*)nullptr, edges, len_sq);
    return hipSuccess;
}

hipError_t launch_refine_children(const int32_t* face, long long nf, const uint8_t* code, const int32_t* foff,
                                  const unsigned int* slot, const unsigned int* own, const double* v, int32_t* out,
                                  hipStream_t s)
{
    MESH_LAUNCH(k_refine_children, mesh_grid(nf), face, nf, code, foff, slot, own, v, out);
    return hipSuccess;
}

}  // namespace mm
