// mm_trim_kernels.hip -- the data-parallel part of CCTA mesh trimming, for gfx950: region membership of every face,
// the open-boundary edge set of the surviving faces, and the compaction of the kept vertices and faces.
//
// remove_labeled_points_from_mesh / keep_labeled_points_from_mesh (multimodars/ccta/stitching.py:110-352),
// open_boundary_edges and the face re-derivation of clean_open_boundary (multimodars/ccta/boundary.py:26-51, 257-325),
// _extract_region_with_border_faces (multimodars/ccta/__init__.py:341-373).  Faces are int32 index triples; every
// index has been checked against [0, nv) on the host.  Masks are uint8 0 / 1 per vertex or per face.
//
//   k_trim_faces         one lane per face.  all-mode: keep = all three corners in `in`; the kept corners of a face that
//                        also has a corner outside `in` are marked (the rim seeds).  any-mode: keep = some corner in
//                        `in`; every corner of a kept face is marked (the used vertices).  Marks are plain byte stores
//                        of 1 from any number of lanes: the races are benign.
//   k_trim_edge_insert   every kept face inserts its three undirected edge keys (min << 32 | max) into the edge table
//                        of mm_mesh_device.h (edge_insert without owners: 64-bit atomicCAS on the key, 32-bit atomicAdd
//                        on its count).  The table holds at least twice as many slots as insertions, so a probe ends.
//   k_trim_edge_compact  the keys of count 1, appended through one returning atomicAdd per wave (wave_append: ballot,
//                        then the lane's rank in the ballot).  The order depends on scheduling; the host sorts the keys,
//                        so the result is the set, independent of it.  No float atomics anywhere.
//   k_trim_tile_count / k_trim_tile_scan / k_trim_index   exclusive scan of a mask (hand-written, three passes: tile
//                        counts, one workgroup scanning the tile counts (scan_tile_sums of mm_mesh_device.h), per-element
//                        indices), -1 where the mask is 0.
//   k_trim_gather / k_trim_remap   the kept vertices to their new slots, the kept faces remapped to the new indices.
//   k_trim_clear         mask[idx[i]] = 0 for the vertices a cleaning round culls.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mm_device.h"
#include "mm_mesh_device.h"

namespace mm {

__global__ void __launch_bounds__(kMeshThreads)
k_trim_faces(const int32_t* __restrict__ face, long long nf, const uint8_t* __restrict__ in, int any_mode,
             uint8_t* __restrict__ fkeep, uint8_t* __restrict__ mark)
{
    for (long long f = mesh_tid(); f < nf; f += mesh_stride()) {
        const int32_t a = face[3 * f], b = face[3 * f + 1], c = face[3 * f + 2];
        const uint8_t ia = in[a], ib = in[b], ic = in[c];
        if (any_mode) {
            const uint8_t k = (ia | ib | ic) ? 1 : 0;
            fkeep[f] = k;
            if (k && mark) { mark[a] = 1; mark[b] = 1; mark[c] = 1; }
        } else {
            const uint8_t k = (ia & ib & ic) ? 1 : 0;
            fkeep[f] = k;
            if (!k && mark) {
                if (ia) mark[a] = 1;
                if (ib) mark[b] = 1;
                if (ic) mark[c] = 1;
            }
        }
    }
}

// the edge table of mm_mesh_device.h without owners: cap = mask + 1 slots, shift = 64 - log2 cap
__global__ void __launch_bounds__(kMeshThreads)
k_trim_edge_insert(const int32_t* __restrict__ face, long long nf, const uint8_t* __restrict__ fkeep,
                   unsigned long long* __restrict__ keys, unsigned int* __restrict__ cnt, unsigned long long mask, int shift)
{
    for (long long f = mesh_tid(); f < nf; f += mesh_stride()) {
        if (!fkeep[f]) continue;
        const int32_t a = face[3 * f], b = face[3 * f + 1], c = face[3 * f + 2];
        edge_insert<false>(keys, cnt, nullptr, mask, shift, a, b, 0u);
        edge_insert<false>(keys, cnt, nullptr, mask, shift, b, c, 0u);
        edge_insert<false>(keys, cnt, nullptr, mask, shift, c, a, 0u);
    }
}

// cap is a multiple of kMeshThreads and the stride a multiple of it: every wave runs the loop with all 64 lanes
__global__ void __launch_bounds__(kMeshThreads)
k_trim_edge_compact(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ cnt,
                    unsigned long long cap, unsigned long long* __restrict__ out, unsigned long long* __restrict__ n_out)
{
    for (unsigned long long s = (unsigned long long)mesh_tid(); s < cap; s += (unsigned long long)mesh_stride()) {
        const unsigned long long k = keys[s];
        const bool open = k != kEdgeEmpty && cnt[s] == 1u;
        const unsigned long long at = wave_append(open, n_out);
        if (open) out[at] = k;
    }
}

// tile_sum[t] = the number of nonzero flags in tile t (kScanTile flags); grid = the number of tiles
__global__ void __launch_bounds__(kMeshThreads)
k_trim_tile_count(const uint8_t* __restrict__ flag, long long n, long long* __restrict__ tile_sum)
{
    const long long i0 = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
    long long c = 0;
    for (int j = 0; j < kScanItems; ++j)
        if (i0 + j < n) c += flag[i0 + j] != 0;
    long long total;
    block_exclusive<kMeshThreads>(c, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

// one workgroup: tile_sum -> exclusive offsets in place, tile_sum[n_tiles] = the total
__global__ void __launch_bounds__(kMeshThreads)
k_trim_tile_scan(long long* __restrict__ tile_sum, long long n_tiles)
{
    const long long total = scan_tile_sums(tile_sum, n_tiles);
    if (threadIdx.x == 0) tile_sum[n_tiles] = total;
}

// idx[i] = the number of nonzero flags before i where flag[i] != 0, else -1
__global__ void __launch_bounds__(kMeshThreads)
k_trim_index(const uint8_t* __restrict__ flag, long long n, const long long* __restrict__ tile_off,
             int32_t* __restrict__ idx)
{
    const long long i0 = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
    long long c = 0;
    for (int j = 0; j < kScanItems; ++j)
        if (i0 + j < n) c += flag[i0 + j] != 0;
    long long total;
    long long at = tile_off[blockIdx.x] + block_exclusive<kMeshThreads>(c, &total);
    for (int j = 0; j < kScanItems; ++j) {
        if (i0 + j >= n) break;
        if (flag[i0 + j]) idx[i0 + j] = (int32_t)at++;
        else idx[i0 + j] = -1;
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_trim_gather(const double* __restrict__ v, long long nv, const int32_t* __restrict__ vidx, double* __restrict__ out)
{
    for (long long i = mesh_tid(); i < nv; i += mesh_stride()) {
        const int32_t k = vidx[i];
        if (k < 0) continue;
        out[3 * (long long)k] = v[3 * i];
        out[3 * (long long)k + 1] = v[3 * i + 1];
        out[3 * (long long)k + 2] = v[3 * i + 2];
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_trim_remap(const int32_t* __restrict__ face, long long nf, const int32_t* __restrict__ fidx,
             const int32_t* __restrict__ vidx, int32_t* __restrict__ out)
{
    for (long long f = mesh_tid(); f < nf; f += mesh_stride()) {
        const int32_t k = fidx[f];
        if (k < 0) continue;
        out[3 * (long long)k] = vidx[face[3 * f]];
        out[3 * (long long)k + 1] = vidx[face[3 * f + 1]];
        out[3 * (long long)k + 2] = vidx[face[3 * f + 2]];
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_trim_clear(const int32_t* __restrict__ idx, long long n, uint8_t* __restrict__ mask)
{
    for (long long i = mesh_tid(); i < n; i += mesh_stride()) mask[idx[i]] = 0;
}

hipError_t launch_trim_faces(const int32_t* face, long long nf, const uint8_t* in, int any_mode, uint8_t* fkeep,
                             uint8_t* mark, hipStream_t s)
{
    if (nf > 0) MESH_LAUNCH(k_trim_faces, mesh_grid(nf), face, nf, in, any_mode, fkeep, mark);
    return hipSuccess;
}

hipError_t launch_trim_open_edges(const int32_t* face, long long nf, const uint8_t* fkeep, unsigned long long* keys,
                                  unsigned int* cnt, int log2_cap, unsigned long long* out, unsigned long long* n_out,
                                  hipStream_t s)
{
    const unsigned long long cap = 1ull << log2_cap;
    hipError_t he;
    if ((he = hipMemsetAsync(keys, 0xFF, cap * 8, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(cnt, 0, cap * 4, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(n_out, 0, 8, s)) != hipSuccess) return he;
    if (nf <= 0) return hipSuccess;
    MESH_LAUNCH(k_trim_edge_insert, mesh_grid(nf), face, nf, fkeep, keys, cnt, cap - 1, 64 - log2_cap);
    MESH_LAUNCH(k_trim_edge_compact, mesh_grid((long long)cap), keys, cnt, cap, out, n_out);
    return hipSuccess;
}

size_t trim_scan_tiles(long long n) { return scan_tiles(n); }

hipError_t launch_trim_scan(const uint8_t* flag, long long n, long long* tile_sum, int32_t* idx, hipStream_t s)
{
    const long long tiles = (long long)scan_tiles(n);
    if (tiles == 0) return hipMemsetAsync(tile_sum, 0, 8, s);
    MESH_LAUNCH(k_trim_tile_count, (unsigned)tiles, flag, n, tile_sum);
    MESH_LAUNCH(k_trim_tile_scan, 1u, tile_sum, tiles);
    MESH_LAUNCH(k_trim_index, (unsigned)tiles, flag, n, tile_sum, idx);
    return hipSuccess;
}

hipError_t launch_trim_compact(const double* v, long long nv, const int32_t* vidx, const int32_t* face, long long nf,
                               const int32_t* fidx, double* out_v, int32_t* out_f, hipStream_t s)
{
    if (nv > 0) MESH_LAUNCH(k_trim_gather, mesh_grid(nv), v, nv, vidx, out_v);
    if (nf > 0) MESH_LAUNCH(k_trim_remap, mesh_grid(nf), face, nf, fidx, vidx, out_f);
    return hipSuccess;
}

hipError_t launch_trim_clear(const int32_t* idx, long long n, uint8_t* mask, hipStream_t s)
{
    if (n > 0) MESH_LAUNCH(k_trim_clear, mesh_grid(n), idx, n, mask);
    return hipSuccess;
}

}  // namespace mm
