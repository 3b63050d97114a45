// mm_geodesic_kernels.hip -- the geodesic distance field over the edge graph of a mesh, for gfx950
// (include/mm_centerline.h, "Rule G").
//
// The field is the least fixpoint of d[v] = min(d[v], fl(d[u] + w(u, v))) from d = +0.0 at the seeds and +inf elsewhere.
// Rounded addition of a non-negative weight is monotone, so that fixpoint is unique and every order of relaxations that
// reaches it gives the same bits: the schedule below is free, and nothing in it depends on which lane arrives first.
//
//   k_geo_weights   one lane per vertex: the weight of every entry of its row of the sorted adjacency (launch_mesh_csr),
//                   from the edge's (lo, hi) ends in that order, so both directions hold the same bits; an edge whose
//                   weight is not finite gets +inf, which no relaxation can use, and is counted once, at its lower end.
//                   The longest finite weight as an integer atomicMax on its bits, one per wave.
//   k_geo_init / k_geo_seed   dist = +inf, seed bytes and block flags 0; then one lane per seed: dist = +0.0, the seed
//                   byte, and the flag of its own block of 256 vertices and of every neighbour's block.
//   k_geo_round     one workgroup per flagged block of 256 consecutive vertices.  The block's distances go to LDS and the
//                   workgroup relaxes them to a LOCAL fixpoint (each lane pulls over its own row: neighbours inside the
//                   block from LDS, outside through 8-byte relaxed atomic loads; the first 8 entries of the row are held
//                   in registers, so a sweep of the loop is LDS reads, adds and one barrier), then publishes what fell with 8-byte
//                   relaxed atomic stores -- a vertex is written by its own block alone -- and flags, for the next round,
//                   the blocks of the outside neighbours of every vertex that fell.  A block that read a neighbour before
//                   its owner published it was flagged by that owner, so it runs again: when a round flags nothing the
//                   field is the fixpoint.  The flags alternate between two arrays; round r counts the blocks it flagged
//                   in marks[r], which the host reads once per batch of rounds.
//   k_geo_pred      one lane per vertex, after convergence: the smallest neighbour u with fl(dist[u] + w) == dist[v] (the
//                   row is ascending, so the first), -1 at seeds and unreached vertices; the vertices reached (ballot) and
//                   the largest finite distance (integer atomicMax on the bits).
//
// No floating-point atomics; non-negative doubles order like their bits.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mm_device.h"
#include "mm_mesh_device.h"

namespace mm {

static constexpr unsigned long long kGeoInf = 0x7FF0000000000000ull;          // the bits of +inf
static constexpr int kGeoRow = 8;                                              // row entries a lane of k_geo_round keeps in registers

static __device__ __forceinline__ double geo_load(const unsigned long long* p)
{
    return __longlong_as_double((long long)__atomic_load_n(p, __ATOMIC_RELAXED));
}

__global__ void __launch_bounds__(kMeshThreads)
k_geo_weights(const double* __restrict__ v, const int32_t* __restrict__ off, const int32_t* __restrict__ nb,
              long long nv_padded, long long nv, double* __restrict__ w, unsigned long long* __restrict__ counts)
{
    for (long long i = mesh_tid(); i < nv_padded; i += mesh_stride()) {
        unsigned long long longest = 0;
        int skipped = 0;
        if (i < nv) {
            for (int32_t k = off[i], e = off[i + 1]; k < e; ++k) {
                const long long u = nb[k];
                const double* lo = v + 3 * (u < i ? u : i);
                const double* hi = v + 3 * (u < i ? i : u);
                const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
                double x = sqrt((dx * dx + dy * dy) + dz * dz);
                const unsigned long long bits = (unsigned long long)__double_as_longlong(x);
                if (bits >= kGeoInf) {                                  // +inf or NaN (a square root is never negative)
                    x = __longlong_as_double((long long)kGeoInf);
                    skipped += i < u;
                } else if (bits > longest) {
                    longest = bits;
                }
                w[k] = x;
            }
        }
        for (int s = 1; s < 64; s <<= 1) {
            skipped += __shfl_xor(skipped, s);
            const unsigned long long other = (unsigned long long)__shfl_xor((long long)longest, s);
            longest = other > longest ? other : longest;
        }
        if (__lane_id() == 0) {
            if (skipped) atomicAdd(&counts[geo_num_skipped], (unsigned long long)skipped);
            if (longest) atomicMax(&counts[geo_num_max_edge], longest);
        }
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_geo_init(unsigned long long* __restrict__ dist, uint8_t* __restrict__ is_seed, long long nv)
{
    for (long long i = mesh_tid(); i < nv; i += mesh_stride()) {
        dist[i] = kGeoInf;
        is_seed[i] = 0;
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_geo_seed(const int32_t* __restrict__ seeds, long long n, const int32_t* __restrict__ off, const int32_t* __restrict__ nb,
           unsigned long long* __restrict__ dist, uint8_t* __restrict__ is_seed, unsigned int* __restrict__ flag)
{
    for (long long i = mesh_tid(); i < n; i += mesh_stride()) {
        const int32_t sv = seeds[i];
        __atomic_store_n(&dist[sv], 0ull, __ATOMIC_RELAXED);            // a repeated seed writes the same bits
        is_seed[sv] = 1;
        __atomic_store_n(&flag[sv / kMeshThreads], 1u, __ATOMIC_RELAXED);
        for (int32_t k = off[sv], e = off[sv + 1]; k < e; ++k)
            __atomic_store_n(&flag[nb[k] / kMeshThreads], 1u, __ATOMIC_RELAXED);
    }
}

// one round: cur = the flags this round consumes (each cleared by its own block), next = those it raises (all 0 before)
__global__ void __launch_bounds__(kMeshThreads)
k_geo_round(const int32_t* __restrict__ off, const int32_t* __restrict__ nb, const double* __restrict__ w, long long nv,
            long long n_blocks, unsigned long long* __restrict__ dist, unsigned int* __restrict__ cur,
            unsigned int* __restrict__ next, unsigned long long* __restrict__ mark)
{
    __shared__ double s_d[2][kMeshThreads];
    __shared__ int s_fell[2][kMeshThreads / 64];                          // whether a wave's lanes fell, by the sweep's parity
    const double inf = __longlong_as_double((long long)kGeoInf);
    for (long long b = blockIdx.x; b < n_blocks; b += gridDim.x) {
        if (__atomic_load_n(&cur[b], __ATOMIC_RELAXED) == 0) continue;          // uniform over the workgroup
        __syncthreads();                                                 // every lane has read the flag
        if (threadIdx.x == 0) __atomic_store_n(&cur[b], 0u, __ATOMIC_RELAXED);
        const long long base = b * kMeshThreads, i = base + threadIdx.x;
        const bool live = i < nv;
        const double before = live ? geo_load(&dist[i]) : 0.0;
        const int32_t r0 = live ? off[i] : 0, r1 = live ? off[i + 1] : 0;
        // the first kGeoRow entries of the row stay in registers: where the neighbour sits in LDS, or its distance as it
        // is now (its owner flags this block when it falls), and the weight; an absent entry adds +inf, which never wins
        int32_t at[kGeoRow];
        double wr[kGeoRow], ex[kGeoRow];
#pragma unroll
        for (int j = 0; j < kGeoRow; ++j) {
            at[j] = -1;
            wr[j] = inf;
            ex[j] = inf;
            if (r0 + j < r1) {
                const long long u = nb[r0 + j];
                const long long local = u - base;
                wr[j] = w[r0 + j];
                if (local >= 0 && local < kMeshThreads) at[j] = (int32_t)local;
                else ex[j] = geo_load(&dist[u]);
            }
        }
        double mine = before;
        int p = 0;
        s_d[0][threadIdx.x] = mine;
        __syncthreads();
        for (;;) {                                                       // reads s_d[p], writes s_d[1 - p]: one barrier a sweep
            double best = mine;
#pragma unroll
            for (int j = 0; j < kGeoRow; ++j) {
                const double c = (at[j] >= 0 ? s_d[p][at[j]] : ex[j]) + wr[j];
                best = c < best ? c : best;
            }
            for (int32_t k = r0 + kGeoRow; k < r1; ++k) {                 // a long row (a fan's centre): from memory
                const long long u = nb[k];
                const long long local = u - base;
                const double du = (local >= 0 && local < kMeshThreads) ? s_d[p][local] : geo_load(&dist[u]);
                const double c = du + w[k];
                best = c < best ? c : best;
            }
            const bool fell = best < mine;
            mine = best;
            s_d[1 - p][threadIdx.x] = mine;
            const unsigned long long wave_fell = __ballot(fell);
            if (__lane_id() == 0) s_fell[p][threadIdx.x >> 6] = wave_fell != 0;
            __syncthreads();
            const int any = s_fell[p][0] | s_fell[p][1] | s_fell[p][2] | s_fell[p][3];
            p = 1 - p;
            if (!any) break;
        }
        int raised = 0;
        if (live && mine < before) {
            __atomic_store_n(&dist[i], (unsigned long long)__double_as_longlong(mine), __ATOMIC_RELAXED);
            for (int32_t k = r0; k < r1; ++k) {
                const long long ub = nb[k] / kMeshThreads;
                if (ub != b && __atomic_exchange_n(&next[ub], 1u, __ATOMIC_RELAXED) == 0) ++raised;
            }
        }
        if (raised) atomicAdd(mark, (unsigned long long)raised);
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_geo_pred(const int32_t* __restrict__ off, const int32_t* __restrict__ nb, const double* __restrict__ w,
           const unsigned long long* __restrict__ dist, const uint8_t* __restrict__ is_seed, long long nv_padded,
           long long nv, int32_t* __restrict__ pred, unsigned long long* __restrict__ counts)
{
    for (long long i = mesh_tid(); i < nv_padded; i += mesh_stride()) {
        unsigned long long bits = 0;
        bool reached = false;
        if (i < nv) {
            bits = dist[i];
            reached = bits < kGeoInf;
            int32_t p = -1;
            if (reached && !is_seed[i]) {
                const double d = __longlong_as_double((long long)bits);
                for (int32_t k = off[i], e = off[i + 1]; k < e; ++k) {
                    const int32_t u = nb[k];
                    if (__longlong_as_double((long long)dist[u]) + w[k] == d) {
                        p = u;
                        break;
                    }
                }
            }
            pred[i] = p;
            if (!reached) bits = 0;
        }
        wave_count(reached, &counts[geo_num_reached]);
        for (int s = 1; s < 64; s <<= 1) {
            const unsigned long long other = (unsigned long long)__shfl_xor((long long)bits, s);
            bits = other > bits ? other : bits;
        }
        if (__lane_id() == 0 && bits) atomicMax(&counts[geo_num_max_dist], bits);
    }
}

size_t geo_blocks(long long nv) { return (size_t)((nv + kMeshThreads - 1) / kMeshThreads); }

hipError_t launch_geo_weights(const double* v, const int32_t* off, const int32_t* nb, long long nv, double* w,
                              unsigned long long* counts, hipStream_t s)
{
    MESH_LAUNCH(k_geo_weights, mesh_grid(nv), v, off, nb, mesh_pad(nv), nv, w, counts);
    return hipSuccess;
}

hipError_t launch_geo_seed(const int32_t* seeds, long long n_seeds, const int32_t* off, const int32_t* nb, long long nv,
                           unsigned long long* dist, uint8_t* is_seed, unsigned int* flag_a, unsigned int* flag_b,
                           hipStream_t s)
{
    hipError_t he;
    const size_t fb = geo_blocks(nv) * 4;
    if ((he = hipMemsetAsync(flag_a, 0, fb, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(flag_b, 0, fb, s)) != hipSuccess) return he;
    MESH_LAUNCH(k_geo_init, mesh_grid(nv), dist, is_seed, nv);
    MESH_LAUNCH(k_geo_seed, mesh_grid(n_seeds), seeds, n_seeds, off, nb, dist, is_seed, flag_a);
    return hipSuccess;
}

hipError_t launch_geo_round(const int32_t* off, const int32_t* nb, const double* w, long long nv, unsigned long long* dist,
                            unsigned int* cur, unsigned int* next, unsigned long long* mark, hipStream_t s)
{
    const long long n_blocks = (long long)geo_blocks(nv);
    MESH_LAUNCH(k_geo_round, (unsigned)(n_blocks > 65536 ? 65536 : n_blocks), off, nb, w, nv, n_blocks, dist, cur, next, mark);
    return hipSuccess;
}

hipError_t launch_geo_pred(const int32_t* off, const int32_t* nb, const double* w, const unsigned long long* dist,
                           const uint8_t* is_seed, long long nv, int32_t* pred, unsigned long long* counts, hipStream_t s)
{
    MESH_LAUNCH(k_geo_pred, mesh_grid(nv), off, nb, w, dist, is_seed, mesh_pad(nv), nv, pred, counts);
    return hipSuccess;
}


// ---- Rule S: the nodes of the band skeleton.  Every result below is a function of the input alone: integer atomics
// build unordered lists, a sort puts each in order, and every floating-point sum is one lane walking a sorted list. ----

// band[i] = (int64)(dist / h), -1 where dist is +inf; counts[band_over] set where a quotient reaches 2^31; link[i] = i << 1
__global__ void __launch_bounds__(kMeshThreads)
k_skel_band(const unsigned long long* __restrict__ dist, long long nv, double h, int32_t* __restrict__ band,
            unsigned int* __restrict__ link, unsigned long long* __restrict__ counts)
{
    for (long long i = mesh_tid(); i < nv; i += mesh_stride()) {
        const unsigned long long bits = dist[i];
        int32_t b = -1;
        if (bits < kGeoInf) {
            const double q = __longlong_as_double((long long)bits) / h;
            if (q >= 2147483648.0) counts[geo_num_band_over] = 1;
            else b = (int32_t)(long long)q;
        }
        band[i] = b;
        link[i] = (unsigned int)i << 1;
    }
}

// the vertices of one band joined across the graph's edges: the root of a set ends as its smallest vertex
__global__ void __launch_bounds__(kMeshThreads)
k_skel_hook(const int32_t* __restrict__ off, const int32_t* __restrict__ nb, const double* __restrict__ w,
            const int32_t* __restrict__ band, long long nv, unsigned int* __restrict__ link)
{
    for (long long i = mesh_tid(); i < nv; i += mesh_stride()) {
        const int32_t bi = band[i];
        if (bi < 0) continue;
        for (int32_t k = off[i], e = off[i + 1]; k < e; ++k) {
            const int32_t u = nb[k];
            if (u > i && (unsigned long long)__double_as_longlong(w[k]) < kGeoInf && band[u] == bi)
                uf_union(link, (unsigned int)i, (unsigned int)u, 0u);
        }
    }
}

// behind the flattening rounds: is_root[i] = i stands for a node
__global__ void __launch_bounds__(kMeshThreads)
k_skel_roots(const unsigned int* __restrict__ link, const int32_t* __restrict__ band, long long nv, uint8_t* __restrict__ is_root)
{
    for (long long i = mesh_tid(); i < nv; i += mesh_stride()) is_root[i] = band[i] >= 0 && (link[i] >> 1) == (unsigned int)i;
}

// keys[ridx[i]] = band << 32 | i at the roots; the entries from n_keys to n_padded (a power of two) = ~0
__global__ void __launch_bounds__(kMeshThreads)
k_skel_keys(const int32_t* __restrict__ ridx, const int32_t* __restrict__ band, long long nv, long long n_keys,
            long long n_padded, unsigned long long* __restrict__ keys)
{
    for (long long i = mesh_tid(); i < nv || i < n_padded; i += mesh_stride()) {
        if (i < nv && ridx[i] >= 0) keys[ridx[i]] = ((unsigned long long)(unsigned int)band[i] << 32) | (unsigned long long)i;
        if (i >= n_keys && i < n_padded) keys[i] = ~0ull;
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_geo_pad(unsigned long long* __restrict__ keys, long long from, long long to)
{
    for (long long i = from + mesh_tid(); i < to; i += mesh_stride()) keys[i] = ~0ull;
}

// one compare-exchange step of the bitonic network over n (a power of two) distinct keys, ascending
__global__ void __launch_bounds__(kMeshThreads)
k_geo_bitonic(unsigned long long* __restrict__ keys, long long n, long long j, long long k)
{
    for (long long i = mesh_tid(); i < n; i += mesh_stride()) {
        const long long l = i ^ j;
        if (l <= i) continue;
        const unsigned long long a = keys[i], b = keys[l];
        if (((i & k) == 0) == (a > b)) {
            keys[i] = b;
            keys[l] = a;
        }
    }
}

// node_of_root[the vertex in key p] = p
__global__ void __launch_bounds__(kMeshThreads)
k_skel_number(const unsigned long long* __restrict__ keys, long long n_nodes, int32_t* __restrict__ node_of_root)
{
    for (long long p = mesh_tid(); p < n_nodes; p += mesh_stride()) node_of_root[keys[p] & 0xFFFFFFFFull] = (int32_t)p;
}

// vnode; the node's flag bits 0 (a rim vertex that is no seed) and 2 (a seed); its numbers of vertices and corners
__global__ void __launch_bounds__(kMeshThreads)
k_skel_vertex_node(const unsigned int* __restrict__ link, const int32_t* __restrict__ band,
                   const int32_t* __restrict__ node_of_root, const uint8_t* __restrict__ rim,
                   const uint8_t* __restrict__ is_seed, long long nv, int32_t* __restrict__ vnode,
                   unsigned int* __restrict__ nflags, int32_t* __restrict__ vcnt)
{
    for (long long i = mesh_tid(); i < nv; i += mesh_stride()) {
        int32_t n = -1;
        if (band[i] >= 0) {
            n = node_of_root[link[i] >> 1];
            const unsigned int bits = (rim[i] && !is_seed[i] ? 1u : 0u) | (is_seed[i] ? 4u : 0u);
            if (bits) atomicOr(&nflags[n], bits);
            atomicAdd(&vcnt[n], 1);
        }
        vnode[i] = n;
    }
}

// rim[lo] = rim[hi] = 1 for every edge between different vertices that one corner of one face inserted
__global__ void __launch_bounds__(kMeshThreads)
k_skel_rim(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ cnt, unsigned long long cap,
           uint8_t* __restrict__ rim)
{
    for (unsigned long long s = (unsigned long long)mesh_tid(); s < cap; s += (unsigned long long)mesh_stride()) {
        const unsigned long long k = keys[s];
        if (k == kEdgeEmpty || cnt[s] != 1u || edge_lo(k) == edge_hi(k)) continue;
        rim[edge_lo(k)] = 1;
        rim[edge_hi(k)] = 1;
    }
}

// area3[f] = a_f / 3; ccnt[node of the corner] += 1
__global__ void __launch_bounds__(kMeshThreads)
k_skel_faces(const double* __restrict__ v, const int32_t* __restrict__ face, long long nf, const int32_t* __restrict__ vnode,
             double* __restrict__ area3, int32_t* __restrict__ ccnt)
{
    for (long long f = mesh_tid(); f < nf; f += mesh_stride()) {
        const int32_t i0 = face[3 * f], i1 = face[3 * f + 1], i2 = face[3 * f + 2];
        const double *p0 = v + 3 * (long long)i0, *p1 = v + 3 * (long long)i1, *p2 = v + 3 * (long long)i2;
        const double ax = p1[0] - p0[0], ay = p1[1] - p0[1], az = p1[2] - p0[2];
        const double bx = p2[0] - p0[0], by = p2[1] - p0[1], bz = p2[2] - p0[2];
        const double cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
        area3[f] = (0.5 * sqrt((cx * cx + cy * cy) + cz * cz)) / 3.0;
        if (vnode[i0] >= 0) atomicAdd(&ccnt[vnode[i0]], 1);
        if (vnode[i1] >= 0) atomicAdd(&ccnt[vnode[i1]], 1);
        if (vnode[i2] >= 0) atomicAdd(&ccnt[vnode[i2]], 1);
    }
}

// the unordered lists: the corners and the vertices of every node, through the rows' cursors
__global__ void __launch_bounds__(kMeshThreads)
k_skel_fill(const int32_t* __restrict__ face, long long nf, const int32_t* __restrict__ vnode, long long nv,
            int32_t* __restrict__ ccur, int32_t* __restrict__ clist, int32_t* __restrict__ vcur, int32_t* __restrict__ vlist)
{
    for (long long i = mesh_tid(); i < 3 * nf || i < nv; i += mesh_stride()) {
        if (i < 3 * nf) {
            const int32_t n = vnode[face[i]];
            if (n >= 0) clist[atomicAdd(&ccur[n], 1)] = (int32_t)i;
        }
        if (i < nv) {
            const int32_t n = vnode[i];
            if (n >= 0) vlist[atomicAdd(&vcur[n], 1)] = (int32_t)i;
        }
    }
}

// one lane per node walks its sorted corners, then its sorted vertices: rec = 10 words a node (x, y, z, radius,
// radius_min, weight as doubles; band, first_vertex, n_vertices, flags as int64)
__global__ void __launch_bounds__(kMeshThreads)
k_skel_nodes(long long n_nodes, const int32_t* __restrict__ coff, const int32_t* __restrict__ clist,
             const int32_t* __restrict__ voff, const int32_t* __restrict__ vlist, const int32_t* __restrict__ face,
             const double* __restrict__ area3, const double* __restrict__ v, const int32_t* __restrict__ band,
             const unsigned int* __restrict__ nflags, double* __restrict__ rec)
{
    for (long long n = mesh_tid(); n < n_nodes; n += mesh_stride()) {
        const int32_t c0 = coff[n], c1 = coff[n + 1], v0 = voff[n], v1 = voff[n + 1];
        double W = 0.0, sx = 0.0, sy = 0.0, sz = 0.0;
        bool bad = false;
        for (int32_t k = c0; k < c1; ++k) {
            const int32_t c = clist[k];
            const double a = area3[c / 3];
            const double* p = v + 3 * (long long)face[c];
            bad |= (unsigned long long)__double_as_longlong(a) >= kGeoInf;          // a is never negative
            W = W + a;
            sx = sx + a * p[0];
            sy = sy + a * p[1];
            sz = sz + a * p[2];
        }
        const bool plain = bad || !(W > 0.0);
        const double count = (double)(v1 - v0);
        if (plain) {
            sx = sy = sz = 0.0;
            for (int32_t k = v0; k < v1; ++k) {
                const double* p = v + 3 * (long long)vlist[k];
                sx = sx + p[0];
                sy = sy + p[1];
                sz = sz + p[2];
            }
        }
        const double div = plain ? count : W;
        const double x = sx / div, y = sy / div, z = sz / div;
        double R = 0.0, least = __longlong_as_double((long long)kGeoInf);
        if (!plain) {
            for (int32_t k = c0; k < c1; ++k) {
                const int32_t c = clist[k];
                const double* p = v + 3 * (long long)face[c];
                const double dx = p[0] - x, dy = p[1] - y, dz = p[2] - z;
                R = R + area3[c / 3] * sqrt((dx * dx + dy * dy) + dz * dz);
            }
        }
        for (int32_t k = v0; k < v1; ++k) {
            const double* p = v + 3 * (long long)vlist[k];
            const double dx = p[0] - x, dy = p[1] - y, dz = p[2] - z;
            const double r = sqrt((dx * dx + dy * dy) + dz * dz);
            if (plain) R = R + r;
            least = r < least ? r : least;
        }
        double* o = rec + 10 * n;
        long long* oi = (long long*)o;
        o[0] = x; o[1] = y; o[2] = z;
        o[3] = R / div;
        o[4] = least;
        o[5] = plain ? 0.0 : W;
        oi[6] = band[vlist[v0]];
        oi[7] = vlist[v0];
        oi[8] = v1 - v0;
        oi[9] = (long long)(nflags[n] | (plain ? 2u : 0u));
    }
}

// the pairs of different nodes an edge of the graph joins, into a table cleared before
__global__ void __launch_bounds__(kMeshThreads)
k_skel_edge_insert(const int32_t* __restrict__ off, const int32_t* __restrict__ nb, const double* __restrict__ w,
                   const int32_t* __restrict__ vnode, long long nv, unsigned long long* __restrict__ keys,
                   unsigned long long mask, int shift)
{
    for (long long i = mesh_tid(); i < nv; i += mesh_stride()) {
        const int32_t ni = vnode[i];
        if (ni < 0) continue;
        for (int32_t k = off[i], e = off[i + 1]; k < e; ++k) {
            const int32_t u = nb[k];
            if (u < i || (unsigned long long)__double_as_longlong(w[k]) >= kGeoInf) continue;
            const int32_t nu = vnode[u];
            if (nu >= 0 && nu != ni) edge_claim(keys, mask, shift, ni, nu);
        }
    }
}

// the table's keys into out, in no fixed order; cap is a multiple of the workgroup, as is the stride
__global__ void __launch_bounds__(kMeshThreads)
k_skel_edge_compact(const unsigned long long* __restrict__ keys, unsigned long long cap, unsigned long long* __restrict__ out,
                    unsigned long long* __restrict__ n_out)
{
    for (unsigned long long s = (unsigned long long)mesh_tid(); s < cap; s += (unsigned long long)mesh_stride()) {
        const unsigned long long k = keys[s];
        const bool there = k != kEdgeEmpty;
        const unsigned long long at = wave_append(there, n_out);
        if (there) out[at] = k;
    }
}

long long geo_sort_size(long long n)
{
    long long p = 2;
    while (p < n) p <<= 1;
    return p;
}

// keys[0 .. n) ascending (distinct keys below ~0); the buffer holds geo_sort_size(n) entries
hipError_t launch_geo_sort(unsigned long long* keys, long long n, int* launches, hipStream_t s)
{
    if (n < 2) return hipSuccess;
    const long long p = geo_sort_size(n);
    if (p > n) {
        MESH_LAUNCH(k_geo_pad, mesh_grid(p - n), keys, n, p);
        ++*launches;
    }
    for (long long k = 2; k <= p; k <<= 1)
        for (long long j = k >> 1; j > 0; j >>= 1) {
            MESH_LAUNCH(k_geo_bitonic, mesh_grid(p), keys, p, j, k);
            ++*launches;
        }
    return hipSuccess;
}

hipError_t launch_skel_bands(const unsigned long long* dist, long long nv, double h, const int32_t* off, const int32_t* nb,
                             const double* w, int32_t* band, unsigned int* link, unsigned long long* counts, hipStream_t s)
{
    MESH_LAUNCH(k_skel_band, mesh_grid(nv), dist, nv, h, band, link, counts);
    MESH_LAUNCH(k_skel_hook, mesh_grid(nv), off, nb, w, band, nv, link);
    return hipSuccess;
}

hipError_t launch_skel_roots(const unsigned int* link, const int32_t* band, long long nv, uint8_t* is_root, hipStream_t s)
{
    MESH_LAUNCH(k_skel_roots, mesh_grid(nv), link, band, nv, is_root);
    return hipSuccess;
}

hipError_t launch_skel_keys(const int32_t* ridx, const int32_t* band, long long nv, long long n_nodes,
                            unsigned long long* keys, hipStream_t s)
{
    MESH_LAUNCH(k_skel_keys, mesh_grid(nv), ridx, band, nv, n_nodes, n_nodes, keys);
    return hipSuccess;
}

hipError_t launch_skel_number(const unsigned long long* keys, long long n_nodes, int32_t* node_of_root,
                              const unsigned long long* ekeys, const unsigned int* ecnt, int log2_cap,
                              const unsigned int* link, const int32_t* band, const uint8_t* is_seed, long long nv,
                              uint8_t* rim, int32_t* vnode, unsigned int* nflags, int32_t* vcnt, int32_t* ccnt, hipStream_t s)
{
    hipError_t he;
    if ((he = hipMemsetAsync(rim, 0, (size_t)nv, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(nflags, 0, (size_t)n_nodes * 4, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(vcnt, 0, (size_t)n_nodes * 4, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(ccnt, 0, (size_t)n_nodes * 4, s)) != hipSuccess) return he;
    MESH_LAUNCH(k_skel_number, mesh_grid(n_nodes), keys, n_nodes, node_of_root);
    MESH_LAUNCH(k_skel_rim, mesh_grid((long long)(1ull << log2_cap)), ekeys, ecnt, 1ull << log2_cap, rim);
    MESH_LAUNCH(k_skel_vertex_node, mesh_grid(nv), link, band, node_of_root, rim, is_seed, nv, vnode, nflags, vcnt);
    return hipSuccess;
}

hipError_t launch_skel_faces(const double* v, const int32_t* face, long long nf, const int32_t* vnode, double* area3,
                             int32_t* ccnt, hipStream_t s)
{
    if (nf > 0) MESH_LAUNCH(k_skel_faces, mesh_grid(nf), v, face, nf, vnode, area3, ccnt);
    return hipSuccess;
}

hipError_t launch_skel_fill(const int32_t* face, long long nf, const int32_t* vnode, long long nv, int32_t* ccur,
                            int32_t* clist, int32_t* vcur, int32_t* vlist, hipStream_t s)
{
    MESH_LAUNCH(k_skel_fill, mesh_grid(3 * nf > nv ? 3 * nf : nv), face, nf, vnode, nv, ccur, clist, vcur, vlist);
    return hipSuccess;
}

hipError_t launch_skel_nodes(long long n_nodes, const int32_t* coff, const int32_t* clist, const int32_t* voff,
                             const int32_t* vlist, const int32_t* face, const double* area3, const double* v,
                             const int32_t* band, const unsigned int* nflags, double* rec, hipStream_t s)
{
    MESH_LAUNCH(k_skel_nodes, mesh_grid(n_nodes), n_nodes, coff, clist, voff, vlist, face, area3, v, band, nflags, rec);
    return hipSuccess;
}

hipError_t launch_skel_edges(const int32_t* off, const int32_t* nb, const double* w, const int32_t* vnode, long long nv,
                             unsigned long long* keys, int log2_cap, unsigned long long* out, unsigned long long* n_out,
                             hipStream_t s)
{
    const unsigned long long cap = 1ull << log2_cap;
    hipError_t he;
    if ((he = hipMemsetAsync(keys, 0xFF, cap * 8, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(n_out, 0, 8, s)) != hipSuccess) return he;
    MESH_LAUNCH(k_skel_edge_insert, mesh_grid(nv), off, nb, w, vnode, nv, keys, cap - 1, 64 - log2_cap);
    MESH_LAUNCH(k_skel_edge_compact, mesh_grid((long long)cap), keys, cap, out, n_out);
    return hipSuccess;
}

}  // namespace mm
