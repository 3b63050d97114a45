// mm_rim_kernels.hip -- the mesh-wide part of the rim conditioning in front of the CCTA stitch, for gfx950.
//
// _prepare_prox_dist_boundary_pts (multimodars/ccta/stitching.py:484-1064) finds ring points on the mesh through a
// {coordinate: index} dict over every vertex (:826, :873), walks two vertex layers out from a few dozen seeds over a
// full adjacency map (:1034-1062) and looks for the faces that own a subdivided rim edge through an edge -> faces dict
// over every face (:881-884, :917-926).  Each of these has an exact answer that does not depend on any order; they run
// here, one lane per vertex or per face, on int32 indices checked by the host.  The ring arithmetic (a few hundred
// points) is host C++ (mm_rim.cpp).  include/mm_ccta.h states the rules.
//
//   k_rim_locate      one lane per vertex: its three f64 bit patterns (-0.0 folded to +0.0; a vertex with a NaN
//                     matches nothing) against R query points staged through LDS kRimChunk at a time (folded by the
//                     host); on a match atomicMax(index[r], v): the last vertex with the coordinates wins, as in a dict.
//   k_rim_write       v[index[i]] = pts[i] where index[i] >= 0 (the host rejects two targets for one vertex).
//   k_rim_mark        arr[index[i]] = i (ring positions) or 0 (layer seeds).
//   k_rim_layer       ring k of the breadth-first layers: a face with a corner of layer k - 1 gives its corners of
//                     layer -1 the layer k with atomicCAS(-1 -> k).  A corner set in this launch reads as k, never as
//                     k - 1, so the result is the BFS layer whatever the scheduling.  *n_new += the vertices set.
//   k_rim_push        a vertex of layer k >= 1 moves by k * step along its radial direction in the plane, unfused,
//                     in the order include/mm_ccta.h states.
//   k_rim_gather      out[i] = v[index[i]].
//   k_rim_edge_faces  keep[f] = 0 and (f, a, b, c) appended to a list when an edge of f joins ring neighbours whose
//                     ring edge receives points; keep[f] = 1 otherwise.
//   k_rim_face_gather the kept faces compacted in input order through launch_trim_scan (the scan of mm_mesh_device.h).
// The only atomics are integer atomics.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mm_device.h"
#include "mm_mesh_device.h"

namespace mm {

static constexpr int kRimChunk = 1024;                                 // query points per LDS chunk: 24 KB

static __device__ __forceinline__ unsigned long long rim_bits(double x)
{
    return (unsigned long long)__double_as_longlong(x == 0.0 ? 0.0 : x);
}

// q: r query points as 3 r bit patterns (x, y, z interleaved), folded; index: r entries, -1 before the launch
__global__ void __launch_bounds__(kMeshThreads)
k_rim_locate(const double* __restrict__ v, long long nv, const unsigned long long* __restrict__ q, int r,
             int32_t* __restrict__ index)
{
    __shared__ unsigned long long s_q[3 * kRimChunk];
    for (long long base = (long long)blockIdx.x * kMeshThreads; base < nv; base += (long long)gridDim.x * kMeshThreads) {
        const long long i = base + threadIdx.x;                        // the trip count is uniform over the block
        bool ok = i < nv;
        unsigned long long bx = 0, by = 0, bz = 0;
        if (ok) {
            const double x = v[3 * i], y = v[3 * i + 1], z = v[3 * i + 2];
            ok = x == x && y == y && z == z;
            bx = rim_bits(x); by = rim_bits(y); bz = rim_bits(z);
        }
        for (int c0 = 0; c0 < r; c0 += kRimChunk) {
            const int m = r - c0 < kRimChunk ? r - c0 : kRimChunk;
            __syncthreads();
            for (int k = threadIdx.x; k < 3 * m; k += kMeshThreads) s_q[k] = q[3 * (long long)c0 + k];
            __syncthreads();
            if (!ok) continue;
            for (int k = 0; k < m; ++k)
                if (s_q[3 * k] == bx && s_q[3 * k + 1] == by && s_q[3 * k + 2] == bz) atomicMax(&index[c0 + k], (int32_t)i);
        }
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_rim_write(const int32_t* __restrict__ index, const double* __restrict__ pts, int n, double* __restrict__ v)
{
    for (long long i = mesh_tid(); i < n; i += mesh_stride()) {
        const long long k = index[i];
        if (k < 0) continue;
        v[3 * k] = pts[3 * i];
        v[3 * k + 1] = pts[3 * i + 1];
        v[3 * k + 2] = pts[3 * i + 2];
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_rim_mark(const int32_t* __restrict__ index, int n, int by_position, int32_t* __restrict__ arr)
{
    for (long long i = mesh_tid(); i < n; i += mesh_stride())
        if (index[i] >= 0) arr[index[i]] = by_position ? (int32_t)i : 0;
}

__global__ void __launch_bounds__(kMeshThreads)
k_rim_layer(const int32_t* __restrict__ face, long long nf, int32_t* __restrict__ layer, int32_t k,
            unsigned int* __restrict__ n_new)
{
    for (long long f = mesh_tid(); f < nf; f += mesh_stride()) {
        const int32_t c[3] = {face[3 * f], face[3 * f + 1], face[3 * f + 2]};
        int32_t l[3];
        for (int j = 0; j < 3; ++j) l[j] = __atomic_load_n(&layer[c[j]], __ATOMIC_RELAXED);
        if (l[0] != k - 1 && l[1] != k - 1 && l[2] != k - 1) continue;
        unsigned int set = 0;
        for (int j = 0; j < 3; ++j)
            if (l[j] == -1 && atomicCAS(&layer[c[j]], -1, k) == -1) ++set;
        if (set) atomicAdd(n_new, set);
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_rim_push(double* __restrict__ v, long long nv, const int32_t* __restrict__ layer, double ox, double oy, double oz,
           double nx, double ny, double nz, double step)
{
    for (long long i = mesh_tid(); i < nv; i += mesh_stride()) {
        const int32_t k = layer[i];
        if (k < 1) continue;
        const double px = v[3 * i], py = v[3 * i + 1], pz = v[3 * i + 2];
        const double d = ((px - ox) * nx + (py - oy) * ny) + (pz - oz) * nz;
        const double rx = (px - d * nx) - ox, ry = (py - d * ny) - oy, rz = (pz - d * nz) - oz;
        const double rn = sqrt((rx * rx + ry * ry) + rz * rz);
        if (rn < 1e-10) continue;
        const double s = ((double)k * step) / rn;
        v[3 * i] = px + s * rx;
        v[3 * i + 1] = py + s * ry;
        v[3 * i + 2] = pz + s * rz;
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_rim_gather(const double* __restrict__ v, const int32_t* __restrict__ index, int n, double* __restrict__ out)
{
    for (long long i = mesh_tid(); i < n; i += mesh_stride()) {
        const long long k = index[i];
        if (k < 0) continue;
        out[3 * i] = v[3 * k];
        out[3 * i + 1] = v[3 * k + 1];
        out[3 * i + 2] = v[3 * k + 2];
    }
}

// the ring edge i joins the ring vertices i and (i + 1) % n and receives counts[i] points
static __device__ __forceinline__ bool rim_edge_splits(int32_t pa, int32_t pb, int n, const int32_t* __restrict__ counts)
{
    if (pa < 0 || pb < 0) return false;
    if ((pa + 1 == n ? 0 : pa + 1) == pb && counts[pa] > 0) return true;
    return (pb + 1 == n ? 0 : pb + 1) == pa && counts[pb] > 0;
}

// list: list_cap entries of 4 words; *n_list counts every touched face, also those beyond list_cap
__global__ void __launch_bounds__(kMeshThreads)
k_rim_edge_faces(const int32_t* __restrict__ face, long long nf, const int32_t* __restrict__ pos,
                 const int32_t* __restrict__ counts, int n, uint8_t* __restrict__ keep, int32_t* __restrict__ list,
                 unsigned int list_cap, unsigned int* __restrict__ n_list)
{
    for (long long f = mesh_tid(); f < nf; f += mesh_stride()) {
        const int32_t a = face[3 * f], b = face[3 * f + 1], c = face[3 * f + 2];
        const int32_t pa = pos[a], pb = pos[b], pc = pos[c];
        const bool touched = rim_edge_splits(pa, pb, n, counts) || rim_edge_splits(pb, pc, n, counts) ||
                             rim_edge_splits(pc, pa, n, counts);
        keep[f] = touched ? 0 : 1;
        if (!touched) continue;
        const unsigned int at = atomicAdd(n_list, 1u);
        if (at >= list_cap) continue;
        list[4 * (size_t)at] = (int32_t)f;
        list[4 * (size_t)at + 1] = a;
        list[4 * (size_t)at + 2] = b;
        list[4 * (size_t)at + 3] = c;
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_rim_face_gather(const int32_t* __restrict__ face, long long nf, const int32_t* __restrict__ fidx, int32_t* __restrict__ out)
{
    for (long long f = mesh_tid(); f < nf; f += mesh_stride()) {
        const long long k = fidx[f];
        if (k < 0) continue;
        out[3 * k] = face[3 * f];
        out[3 * k + 1] = face[3 * f + 1];
        out[3 * k + 2] = face[3 * f + 2];
    }
}

int rim_locate_chunk_points() { return kRimChunk; }

hipError_t launch_rim_locate(const double* v, long long nv, const unsigned long long* q, int r, int32_t* index, hipStream_t s)
{
    MESH_LAUNCH(k_rim_locate, mesh_grid(nv), v, nv, q, r, index);
    return hipSuccess;
}

hipError_t launch_rim_write(const int32_t* index, const double* pts, int n, double* v, hipStream_t s)
{
    MESH_LAUNCH(k_rim_write, mesh_grid(n), index, pts, n, v);
    return hipSuccess;
}

hipError_t launch_rim_mark(const int32_t* index, int n, int by_position, int32_t* arr, hipStream_t s)
{
    MESH_LAUNCH(k_rim_mark, mesh_grid(n), index, n, by_position, arr);
    return hipSuccess;
}

hipError_t launch_rim_layer(const int32_t* face, long long nf, int32_t* layer, int32_t k, unsigned int* n_new, hipStream_t s)
{
    MESH_LAUNCH(k_rim_layer, mesh_grid(nf), face, nf, layer, k, n_new);
    return hipSuccess;
}

hipError_t launch_rim_push(double* v, long long nv, const int32_t* layer, const double o[3], const double n[3], double step,
                           hipStream_t s)
{
    MESH_LAUNCH(k_rim_push, mesh_grid(nv), v, nv, layer, o[0], o[1], o[2], n[0], n[1], n[2], step);
    return hipSuccess;
}

hipError_t launch_rim_gather(const double* v, const int32_t* index, int n, double* out, hipStream_t s)
{
    MESH_LAUNCH(k_rim_gather, mesh_grid(n), v, index, n, out);
    return hipSuccess;
}

hipError_t launch_rim_edge_faces(const int32_t* face, long long nf, const int32_t* pos, const int32_t* counts, int n,
                                 uint8_t* keep, int32_t* list, unsigned int list_cap, unsigned int* n_list, hipStream_t s)
{
    MESH_LAUNCH(k_rim_edge_faces, mesh_grid(nf), face, nf, pos, counts, n, keep, list, list_cap, n_list);
    return hipSuccess;
}

hipError_t launch_rim_face_gather(const int32_t* face, long long nf, const int32_t* fidx, int32_t* out, hipStream_t s)
{
    MESH_LAUNCH(k_rim_face_gather, mesh_grid(nf), face, nf, fidx, out);
    return hipSuccess;
}

}  // namespace mm
