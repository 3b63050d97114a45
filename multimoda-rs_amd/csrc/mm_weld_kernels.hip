// mm_weld_kernels.hip -- the data-parallel part of CCTA stitching, for gfx950: welding the vertices of concatenated
// meshes, dropping repeated and degenerate faces, making the winding consistent and summing the signed volume.
//
// stitch_ccta_to_intravascular (multimodars/ccta/stitching.py:455-468: concatenate, merge_vertices, unique_faces,
// nondegenerate_faces, remove_unreferenced_vertices, _fast_fix_normals) and fix_mesh_winding
// (src/ccta/binding/ccta_py.rs:596-700).  Faces are int32 index triples checked on the host; every stage has an exact,
// order-free answer (include/mm_ccta.h states the rules), so the output does not depend on scheduling.
//
//   k_weld_mark          ref[v] = 1 for every corner of every face (plain byte stores, benign races).
//   k_weld_vertex_insert one lane per referenced vertex with a key (the integer triple rint(c * scale)): an
//                        open-addressing table of int32 slots, each holding the SMALLEST vertex index seen with the
//                        slot's key (first_index_insert of mm_mesh_device.h; a holder's key is re-derived from the
//                        immutable coordinates).  The lane remembers its slot in rep[v].
//   k_weld_vertex_rep    rep[v] = the slot's final value (v itself without a key, -1 unreferenced), keep[v] = rep[v] == v.
//   k_weld_vmap / k_weld_face_insert   vmap[v] = the new index of v's representative; a face with a repeated index
//                        after the weld is dropped, the others go through the same kind of table keyed by their
//                        sorted new index triple.
//   k_weld_face_rep      fkeep[f] = the face is the smallest index of its vertex set.
//   k_weld_edge_insert   the three undirected edges of every face into the edge table of mm_mesh_device.h, with a
//                        count and the first two owners (face << 1 | traverses it from the smaller to the larger end).
//   k_weld_hook          union-find with parity over the edges owned by exactly two faces: link[f] = parent << 1 |
//                        parity to the parent (uf_union of mm_mesh_device.h: the root of a component ends as its
//                        smallest face).
//   k_weld_jump          one round of pointer jumping, link[f] -> its grandparent with the parities added.
//   k_weld_flip          a face of odd parity to its root is reversed (a, b, c) -> (c, b, a); counted per wave.
//   k_weld_edge_report   open, non-manifold and winding-conflict edges of the table, one integer atomicAdd per wave each.
//   k_weld_terms / k_weld_pair_sum   the per-face volume terms and their adjacent-pair tree (a wave's xor-butterfly,
//                        then the four waves through LDS), 256 to 1 per launch.  No float atomics anywhere.
//   k_weld_reverse       every face reversed (the inversion).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mm_device.h"
#include "mm_mesh_device.h"

namespace mm {

// the weld key of one vertex; false where it matches nothing (a non-finite coordinate or a scaled magnitude >= 2^62)
static __device__ __forceinline__ bool weld_key(const double* __restrict__ v, long long i, double scale, long long k[3])
{
    bool ok = true;
    for (int c = 0; c < 3; ++c) {
        const double s = v[3 * i + c] * scale;
        ok = ok && (fabs(s) < 4611686018427387904.0);                 // false for NaN as well
        k[c] = ok ? (long long)rint(s) : 0;
    }
    return ok;
}

__global__ void __launch_bounds__(kMeshThreads)
k_weld_mark(const int32_t* __restrict__ face, long long nf, uint8_t* __restrict__ ref)
{
    for (long long f = mesh_tid(); f < nf; f += mesh_stride()) {
        ref[face[3 * f]] = 1;
        ref[face[3 * f + 1]] = 1;
        ref[face[3 * f + 2]] = 1;
    }
}

// rep[v] = the slot of v's key, -2 for a referenced vertex without a key, -1 unreferenced
__global__ void __launch_bounds__(kMeshThreads)
k_weld_vertex_insert(const double* __restrict__ v, long long nv, const uint8_t* __restrict__ ref, double scale,
                     int32_t* __restrict__ table, unsigned long long mask, int shift, int32_t* __restrict__ rep)
{
    for (long long i = mesh_tid(); i < nv; i += mesh_stride()) {
        if (!ref[i]) { rep[i] = -1; continue; }
        long long k[3];
        if (!weld_key(v, i, scale, k)) { rep[i] = -2; continue; }
        const unsigned long long s = mesh_mix(mesh_mix(mesh_mix(0, (unsigned long long)k[0]), (unsigned long long)k[1]),
                                              (unsigned long long)k[2]) >> shift;
        rep[i] = first_index_insert(table, mask, s, (int32_t)i, [&](int32_t o) {
            long long q[3];
            weld_key(v, o, scale, q);                                  // a holder always has a key
            return q[0] == k[0] && q[1] == k[1] && q[2] == k[2];
        });
    }
}

// counts[0] += the unreferenced vertices (one atomicAdd per wave); nv_padded is a multiple of the workgroup
__global__ void __launch_bounds__(kMeshThreads)
k_weld_vertex_rep(long long nv_padded, long long nv, const int32_t* __restrict__ table, int32_t* __restrict__ rep,
                  uint8_t* __restrict__ keep, unsigned long long* __restrict__ counts)
{
    for (long long i = mesh_tid(); i < nv_padded; i += mesh_stride()) {
        bool unref = false;
        if (i < nv) {
            const int32_t s = rep[i];
            const int32_t r = s >= 0 ? table[s] : (s == -2 ? (int32_t)i : -1);
            rep[i] = r;
            keep[i] = r == (int32_t)i;
            unref = r < 0;
        }
        wave_count(unref, &counts[0]);
    }
}

// vmap[v] = the new index of the vertex v was welded into (-1 unreferenced): vidx is the scan of keep
__global__ void __launch_bounds__(kMeshThreads)
k_weld_vmap(long long nv, const int32_t* __restrict__ rep, const int32_t* __restrict__ vidx, int32_t* __restrict__ vmap)
{
    for (long long i = mesh_tid(); i < nv; i += mesh_stride()) vmap[i] = rep[i] >= 0 ? vidx[rep[i]] : -1;
}

// frep[f] = the slot of f's vertex set in the welded numbering, -1 when two corners coincide there
__global__ void __launch_bounds__(kMeshThreads)
k_weld_face_insert(const int32_t* __restrict__ face, long long nf, const int32_t* __restrict__ vmap,
                   int32_t* __restrict__ table, unsigned long long mask, int shift, int32_t* __restrict__ frep)
{
    for (long long f = mesh_tid(); f < nf; f += mesh_stride()) {
        const int32_t a = vmap[face[3 * f]], b = vmap[face[3 * f + 1]], c = vmap[face[3 * f + 2]];
        if (a == b || b == c || a == c) { frep[f] = -1; continue; }
        int32_t k[3];
        mesh_sort3(a, b, c, k);
        frep[f] = first_index_insert(table, mask, mesh_triple_slot(k, shift), (int32_t)f, [&](int32_t o) {
            int32_t q[3];
            mesh_sort3(vmap[face[3 * (long long)o]], vmap[face[3 * (long long)o + 1]], vmap[face[3 * (long long)o + 2]], q);
            return q[0] == k[0] && q[1] == k[1] && q[2] == k[2];
        });
    }
}

// fkeep[f] = 1 for the survivors; counts[0] += degenerate faces, counts[1] += repeated faces (one atomicAdd per wave)
__global__ void __launch_bounds__(kMeshThreads)
k_weld_face_rep(long long nf_padded, long long nf, const int32_t* __restrict__ table, const int32_t* __restrict__ frep,
                uint8_t* __restrict__ fkeep, unsigned long long* __restrict__ counts)
{
    for (long long f = mesh_tid(); f < nf_padded; f += mesh_stride()) {
        bool degenerate = false, repeated = false;
        if (f < nf) {
            const int32_t s = frep[f];
            degenerate = s < 0;
            repeated = !degenerate && table[s] != (int32_t)f;
            fkeep[f] = !degenerate && !repeated;
        }
        wave_count(degenerate, &counts[0]);
        wave_count(repeated, &counts[1]);
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_weld_edge_insert(const int32_t* __restrict__ face, long long nf, unsigned long long* __restrict__ keys,
                   unsigned int* __restrict__ cnt, unsigned int* __restrict__ own, unsigned long long mask, int shift)
{
    for (long long f = mesh_tid(); f < nf; f += mesh_stride()) {
        const int32_t a = face[3 * f], b = face[3 * f + 1], c = face[3 * f + 2];
        edge_insert<true>(keys, cnt, own, mask, shift, a, b, (unsigned int)f);
        edge_insert<true>(keys, cnt, own, mask, shift, b, c, (unsigned int)f);
        edge_insert<true>(keys, cnt, own, mask, shift, c, a, (unsigned int)f);
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_weld_link_init(unsigned int* __restrict__ link, long long nf)
{
    for (long long f = mesh_tid(); f < nf; f += mesh_stride()) link[f] = (unsigned int)f << 1;
}

__global__ void __launch_bounds__(kMeshThreads)
k_weld_hook(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ cnt,
            const unsigned int* __restrict__ own, unsigned long long cap, unsigned int* __restrict__ link)
{
    for (unsigned long long s = (unsigned long long)mesh_tid(); s < cap; s += (unsigned long long)mesh_stride()) {
        if (keys[s] == kEdgeEmpty || cnt[s] != 2u) continue;
        const unsigned int oa = own[2 * s], ob = own[2 * s + 1];
        unsigned int a = oa >> 1, b = ob >> 1;
        if (a == b) continue;
        uf_union(link, a, b, ((oa ^ ob) & 1u) ^ 1u);                    // same direction: the two faces differ by a flip
    }
}

// one round of pointer jumping; *changed = 1 where a link moved
__global__ void __launch_bounds__(kMeshThreads)
k_weld_jump(unsigned int* __restrict__ link, long long nf, unsigned int* __restrict__ changed)
{
    for (long long f = mesh_tid(); f < nf; f += mesh_stride()) {
        const unsigned int wx = uf_load(&link[f]);
        const unsigned int p = wx >> 1;
        const unsigned int wp = uf_load(&link[p]);
        if ((wp >> 1) != p) {
            __atomic_store_n(&link[f], (wp & ~1u) | ((wx ^ wp) & 1u), __ATOMIC_RELAXED);
            *changed = 1u;
        }
    }
}

// links are flat (every parent a root): reverse the faces of odd parity; *n_flipped += their number
__global__ void __launch_bounds__(kMeshThreads)
k_weld_flip(int32_t* __restrict__ face, long long nf_padded, long long nf, const unsigned int* __restrict__ link,
            unsigned long long* __restrict__ n_flipped)
{
    for (long long f = mesh_tid(); f < nf_padded; f += mesh_stride()) {
        const bool flip = f < nf && (link[f] & 1u);
        if (flip) {
            const int32_t a = face[3 * f], c = face[3 * f + 2];
            face[3 * f] = c;
            face[3 * f + 2] = a;
        }
        wave_count(flip, n_flipped);
    }
}

// counts[0] += edges owned once, counts[1] += edges owned more than twice, counts[2] += edges owned twice whose faces
// (with the flips of `link`, flat) traverse them in the same direction.  cap is a multiple of kMeshThreads.
__global__ void __launch_bounds__(kMeshThreads)
k_weld_edge_report(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ cnt,
                   const unsigned int* __restrict__ own, unsigned long long cap, const unsigned int* __restrict__ link,
                   unsigned long long* __restrict__ counts)
{
    for (unsigned long long s = (unsigned long long)mesh_tid(); s < cap; s += (unsigned long long)mesh_stride()) {
        const bool used = keys[s] != kEdgeEmpty;
        const unsigned int c = used ? cnt[s] : 0u;
        bool conflict = false;
        if (c == 2u) {
            const unsigned int oa = own[2 * s], ob = own[2 * s + 1];
            const unsigned int fa = link ? (link[oa >> 1] & 1u) : 0u, fb = link ? (link[ob >> 1] & 1u) : 0u;
            conflict = (((oa ^ fa) ^ (ob ^ fb)) & 1u) == 0u;
        }
        wave_count(c == 1u, &counts[0]);
        wave_count(c > 2u, &counts[1]);
        wave_count(conflict, &counts[2]);
    }
}

// term[f] = v0 . (v1 x v2), unfused, in the order include/mm_ccta.h states
__global__ void __launch_bounds__(kMeshThreads)
k_weld_terms(const double* __restrict__ v, const int32_t* __restrict__ face, long long nf, double* __restrict__ term)
{
    for (long long f = mesh_tid(); f < nf; f += mesh_stride()) {
        const double* p0 = v + 3 * (long long)face[3 * f];
        const double* p1 = v + 3 * (long long)face[3 * f + 1];
        const double* p2 = v + 3 * (long long)face[3 * f + 2];
        const double cx = p1[1] * p2[2] - p1[2] * p2[1];
        const double cy = p1[2] * p2[0] - p1[0] * p2[2];
        const double cz = p1[0] * p2[1] - p1[1] * p2[0];
        term[f] = (p0[0] * cx + p0[1] * cy) + p0[2] * cz;
    }
}

// out[b] = the adjacent-pair tree over in[256 b .. 256 b + 255], entries at or beyond n reading +0.0.  `levels` (1..8)
// of the tree are summed: fewer than 8 only in the last launch, where the padded length is below 256 (the result is
// then in out[0]; the lanes beyond 2^levels hold other sub-trees and are not read).
__global__ void __launch_bounds__(kMeshThreads)
k_weld_pair_sum(const double* __restrict__ in, long long n, int levels, double* __restrict__ out)
{
    __shared__ double s_wave[kMeshThreads / 64];
    const long long i = (long long)blockIdx.x * kMeshThreads + threadIdx.x;
    double x = i < n ? in[i] : 0.0;
    for (int l = 0; l < 6 && l < levels; ++l) x = x + __shfl_xor(x, 1 << l);
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = x;
    __syncthreads();
    if (threadIdx.x == 0) {
        double r = s_wave[0];
        if (levels > 6) r = s_wave[0] + s_wave[1];
        if (levels > 7) r = r + (s_wave[2] + s_wave[3]);
        out[blockIdx.x] = r;
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_weld_reverse(int32_t* __restrict__ face, long long nf)
{
    for (long long f = mesh_tid(); f < nf; f += mesh_stride()) {
        const int32_t a = face[3 * f], c = face[3 * f + 2];
        face[3 * f] = c;
        face[3 * f + 2] = a;
    }
}

hipError_t launch_weld_vertices(const double* v, long long nv, const int32_t* face, long long nf, double scale,
                                uint8_t* ref, int32_t* table, int log2_cap, int32_t* rep, uint8_t* keep,
                                unsigned long long* counts, hipStream_t s)
{
    const unsigned long long cap = 1ull << log2_cap;
    hipError_t he;
    if ((he = hipMemsetAsync(table, 0xFF, cap * 4, s)) != hipSuccess) return he;
    if (nv <= 0) return hipSuccess;
    if ((he = hipMemsetAsync(ref, 0, (size_t)nv, s)) != hipSuccess) return he;
    if (nf > 0) MESH_LAUNCH(k_weld_mark, mesh_grid(nf), face, nf, ref);
    MESH_LAUNCH(k_weld_vertex_insert, mesh_grid(nv), v, nv, ref, scale, table, cap - 1, 64 - log2_cap, rep);
    MESH_LAUNCH(k_weld_vertex_rep, mesh_grid(nv), mesh_pad(nv), nv, table, rep, keep, counts);
    return hipSuccess;
}

hipError_t launch_weld_faces(const int32_t* face, long long nf, long long nv, const int32_t* rep, const int32_t* vidx,
                             int32_t* vmap, int32_t* table, int log2_cap, int32_t* frep, uint8_t* fkeep,
                             unsigned long long* counts, hipStream_t s)
{
    const unsigned long long cap = 1ull << log2_cap;
    hipError_t he;
    if ((he = hipMemsetAsync(table, 0xFF, cap * 4, s)) != hipSuccess) return he;
    if (nf <= 0) return hipSuccess;
    MESH_LAUNCH(k_weld_vmap, mesh_grid(nv), nv, rep, vidx, vmap);
    MESH_LAUNCH(k_weld_face_insert, mesh_grid(nf), face, nf, vmap, table, cap - 1, 64 - log2_cap, frep);
    MESH_LAUNCH(k_weld_face_rep, mesh_grid(nf), mesh_pad(nf), nf, table, frep, fkeep, counts);
    return hipSuccess;
}

hipError_t launch_weld_edges(const int32_t* face, long long nf, unsigned long long* keys, unsigned int* cnt,
                             unsigned int* own, int log2_cap, hipStream_t s)
{
    const unsigned long long cap = 1ull << log2_cap;
    hipError_t he;
    if ((he = hipMemsetAsync(keys, 0xFF, cap * 8, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(cnt, 0, cap * 4, s)) != hipSuccess) return he;
    if (nf > 0) MESH_LAUNCH(k_weld_edge_insert, mesh_grid(nf), face, nf, keys, cnt, own, cap - 1, 64 - log2_cap);
    return hipSuccess;
}

hipError_t launch_weld_hook(const unsigned long long* keys, const unsigned int* cnt, const unsigned int* own,
                            int log2_cap, unsigned int* link, long long nf, hipStream_t s)
{
    if (nf <= 0) return hipSuccess;
    const unsigned long long cap = 1ull << log2_cap;
    MESH_LAUNCH(k_weld_link_init, mesh_grid(nf), link, nf);
    MESH_LAUNCH(k_weld_hook, mesh_grid((long long)cap), keys, cnt, own, cap, link);
    return hipSuccess;
}

hipError_t launch_weld_jump(unsigned int* link, long long nf, unsigned int* changed, hipStream_t s)
{
    hipError_t he;
    if ((he = hipMemsetAsync(changed, 0, 4, s)) != hipSuccess) return he;
    if (nf > 0) MESH_LAUNCH(k_weld_jump, mesh_grid(nf), link, nf, changed);
    return hipSuccess;
}

hipError_t launch_weld_flip(int32_t* face, long long nf, const unsigned int* link, unsigned long long* n_flipped,
                            hipStream_t s)
{
    if (nf > 0) MESH_LAUNCH(k_weld_flip, mesh_grid(nf), face, mesh_pad(nf), nf, link, n_flipped);
    return hipSuccess;
}

hipError_t launch_weld_edge_report(const unsigned long long* keys, const unsigned int* cnt, const unsigned int* own,
                                   int log2_cap, const unsigned int* link, unsigned long long* counts, hipStream_t s)
{
    const unsigned long long cap = 1ull << log2_cap;                   // at least kMeshThreads (the host sizes it)
    MESH_LAUNCH(k_weld_edge_report, mesh_grid((long long)cap), keys, cnt, own, cap, link, counts);
    return hipSuccess;
}

size_t weld_sum_scratch(long long nf) { return (size_t)((nf + kMeshThreads - 1) / kMeshThreads) + 1; }

// the pair tree over the nf volume terms: the padded length is 2^levels, and a launch sums 8 levels of it
static int weld_tree_levels(long long nf)
{
    int levels = 0;
    while ((1ll << levels) < nf) ++levels;
    return levels;
}
static int weld_tree_launches(int levels) { return levels <= 8 ? 1 : (levels + 7) / 8; }

// the kernels launch_weld_volume launches: the terms, then the tree
int weld_volume_launches(long long nf) { return nf <= 0 ? 0 : 1 + weld_tree_launches(weld_tree_levels(nf)); }

// *out = the adjacent-pair tree of the nf volume terms (padded with +0.0 to a power of two); a and b are scratch of nf
// and weld_sum_scratch(nf) doubles
hipError_t launch_weld_volume(const double* v, const int32_t* face, long long nf, double* a, double* b, double* out,
                              hipStream_t s)
{
    if (nf <= 0) return hipMemsetAsync(out, 0, 8, s);
    MESH_LAUNCH(k_weld_terms, mesh_grid(nf), v, face, nf, a);
    int levels = weld_tree_levels(nf);
    const int launches = weld_tree_launches(levels);
    long long n = nf;
    double* in = a;
    double* to = b;
    for (int k = 1; k <= launches; ++k) {
        const int now = levels >= 8 ? 8 : levels;
        const long long blocks = (n + kMeshThreads - 1) / kMeshThreads;
        MESH_LAUNCH(k_weld_pair_sum, (unsigned)blocks, in, n, now, k == launches ? out : to);
        levels -= 8;
        n = blocks;
        double* t = in; in = to; to = t;
    }
    return hipSuccess;
}

hipError_t launch_weld_reverse(int32_t* face, long long nf, hipStream_t s)
{
    if (nf > 0) MESH_LAUNCH(k_weld_reverse, mesh_grid(nf), face, nf);
    return hipSuccess;
}

}  // namespace mm
