// mm_repair_kernels.hip -- CCTA mesh repair for gfx950: duplicate vertices, degenerate, null and duplicate faces,
// non-manifold edges by removing faces, non-manifold vertices by splitting, unreferenced vertices.
//
// include/mm_ccta.h ("mesh repair") states the rule, tests/mm_checkers/repair_mesh.py is its executable form; the
// reference calls MeshLab for this (multimodars/ccta/fixing_functions.py:114-239).  Every stage has an answer without an
// order of visits, so no output depends on the order in which lanes arrive: the tables keep the smallest index, the edge
// stage keeps the two largest keys (q, face) of an edge through atomicMax, the union-find hooks the larger root under the
// smaller.  One lane per vertex, face, corner or table slot in grid-stride loops; the counters go through wave ballots;
// no LDS but the scans' (launch_trim_scan).  The names a face carries between the stages are the representatives'
// input indices (rep); the output numbering is made once, at the end.
//
//   k_rep_vertex_insert  (a) one lane per vertex: the first-index-wins table of mm_mesh_device.h keyed by the three
//                        coordinates' bit patterns, -0.0 as +0.0; the lane remembers its slot in rep[i].
//   k_rep_vertex_rep     rep[i] = the slot's final value where the weld is on, else i; counts the duplicates.
//   k_rep_face_classify  (b) wf = the face through rep; the cross product and q, unfused; degenerate and null faces
//                        counted; (c) the others into the first-index-wins table keyed by their sorted triple.
//   k_rep_face_rep       fkeep[f] = alive and not a later copy (where that stage is on); counts the copies.
//   k_rep_edge_insert    the edges of the live faces into the edge table, with counts, the first two owners and
//                        eslot[3 f + k] = the slot of the edge leaving corner k.  Runs again behind (d).
//   k_rep_edge_rank      (d) one lane per corner, four launches (phase 0 .. 3) over the slots with more than two owners:
//                        m1q = the largest q (64-bit atomicMax: non-negative doubles order as their bit patterns), m1f =
//                        the largest face with that q, then the same over the owners that are not m1f.
//   k_rep_face_remove    a live face goes iff on some slot with more than two owners it is neither m1f nor m2f; also
//                        link[c] = c << 1 for every corner.
//   k_rep_hook           (e) one lane per slot with exactly two owners: at either end the two owners' corners become one
//                        set (uf_union: the root of a set is its smallest corner).
//   k_rep_vertex_min     links are flat: vmin[x] = the smallest root at vertex x (atomicMin), ref[x] = 1; per INPUT vertex
//                        w the smallest and largest root among its corners (wmin, wmax), per root whether its set holds
//                        corners of more than one input vertex (mixed).
//   k_rep_open           a live root that is not its vertex's minimum: where its set is exactly the corners of one welded
//                        input vertex (not mixed, wmin == wmax == the root) that weld is undone (cback[c], vback[w]);
//                        else it opens a new vertex: isnew[c], vsplit[x].
//   k_rep_vertex_keep    (f) vkeep[i] = a survivor of (a) that is referenced or need not be, or a vertex that came back;
//                        counts.
//   k_rep_out_vertices / k_rep_out_corners   the kept vertices, origin and target; the faces renamed, the new vertices.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mm_device.h"
#include "mm_mesh_device.h"

namespace mm {

// the bit pattern a coordinate is compared by: == on finite doubles, so the two zeros are one
static __device__ __forceinline__ unsigned long long rep_bits(double x)
{
    return x == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(x);
}

__global__ void __launch_bounds__(kMeshThreads)
k_rep_vertex_insert(const double* __restrict__ v, long long nv, int32_t* __restrict__ table, unsigned long long mask,
                    int shift, int32_t* __restrict__ rep)
{
    for (long long i = mesh_tid(); i < nv; i += mesh_stride()) {
        const unsigned long long k0 = rep_bits(v[3 * i]), k1 = rep_bits(v[3 * i + 1]), k2 = rep_bits(v[3 * i + 2]);
        const unsigned long long s = mesh_mix(mesh_mix(mesh_mix(0, k0), k1), k2) >> shift;
        rep[i] = first_index_insert(table, mask, s, (int32_t)i, [&](int32_t o) {
            const double* p = v + 3 * (long long)o;
            return rep_bits(p[0]) == k0 && rep_bits(p[1]) == k1 && rep_bits(p[2]) == k2;
        });
    }
}

// counts[rep_num_welded] += the vertices that are not the first of their coordinates; nv_padded: whole workgroups
__global__ void __launch_bounds__(kMeshThreads)
k_rep_vertex_rep(long long nv_padded, long long nv, const int32_t* __restrict__ table, int weld, int32_t* __restrict__ rep,
                 unsigned long long* __restrict__ counts)
{
    for (long long i = mesh_tid(); i < nv_padded; i += mesh_stride()) {
        bool later = false;
        if (i < nv) {
            const int32_t first = table[rep[i]];
            later = first != (int32_t)i;
            rep[i] = weld ? first : (int32_t)i;
        }
        wave_count(later, &counts[rep_num_welded]);
    }
}

// frep[f] = the slot of f's vertex set, -1 where the face leaves in stage (b)
__global__ void __launch_bounds__(kMeshThreads)
k_rep_face_classify(const int32_t* __restrict__ face, long long nf_padded, long long nf, const int32_t* __restrict__ rep,
                    const double* __restrict__ v, int drop_null, int32_t* __restrict__ table, unsigned long long mask,
                    int shift, int32_t* __restrict__ wf, unsigned long long* __restrict__ qb, int32_t* __restrict__ frep,
                    unsigned long long* __restrict__ counts)
{
    for (long long f = mesh_tid(); f < nf_padded; f += mesh_stride()) {
        bool degenerate = false, null = false;
        if (f < nf) {
            const int32_t a = rep[face[3 * f]], b = rep[face[3 * f + 1]], c = rep[face[3 * f + 2]];
            wf[3 * f] = a; wf[3 * f + 1] = b; wf[3 * f + 2] = c;
            const double *p0 = v + 3 * (long long)a, *p1 = v + 3 * (long long)b, *p2 = v + 3 * (long long)c;
            const double ux = p1[0] - p0[0], uy = p1[1] - p0[1], uz = p1[2] - p0[2];
            const double wx = p2[0] - p0[0], wy = p2[1] - p0[1], wz = p2[2] - p0[2];
            const double cx = uy * wz - uz * wy;
            const double cy = uz * wx - ux * wz;
            const double cz = ux * wy - uy * wx;
            const double q = (cx * cx + cy * cy) + cz * cz;
            qb[f] = (unsigned long long)__double_as_longlong(q);
            degenerate = a == b || b == c || a == c;
            null = !degenerate && cx == 0.0 && cy == 0.0 && cz == 0.0;
            if (degenerate || (null && drop_null)) {
                frep[f] = -1;
            } else {
                int32_t k[3];
                mesh_sort3(a, b, c, k);
                frep[f] = first_index_insert(table, mask, mesh_triple_slot(k, shift), (int32_t)f, [&](int32_t o) {
                    int32_t h[3];                                      // from the immutable inputs: wf[3 o ..] may not be written yet
                    mesh_sort3(rep[face[3 * (long long)o]], rep[face[3 * (long long)o + 1]], rep[face[3 * (long long)o + 2]], h);
                    return h[0] == k[0] && h[1] == k[1] && h[2] == k[2];
                });
            }
        }
        wave_count(degenerate, &counts[rep_num_degenerate]);
        wave_count(null, &counts[rep_num_null]);
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_rep_face_rep(long long nf_padded, long long nf, const int32_t* __restrict__ table, const int32_t* __restrict__ frep,
               int drop_copies, uint8_t* __restrict__ fkeep, unsigned long long* __restrict__ counts)
{
    for (long long f = mesh_tid(); f < nf_padded; f += mesh_stride()) {
        bool copy = false;
        if (f < nf) {
            const int32_t s = frep[f];
            copy = s >= 0 && table[s] != (int32_t)f;
            fkeep[f] = s >= 0 && !(copy && drop_copies);
        }
        wave_count(copy, &counts[rep_num_copies]);
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_rep_edge_insert(const int32_t* __restrict__ wf, long long nf, const uint8_t* __restrict__ fkeep,
                  unsigned long long* __restrict__ keys, unsigned int* __restrict__ cnt, unsigned int* __restrict__ own,
                  unsigned long long mask, int shift, unsigned int* __restrict__ eslot)
{
    for (long long f = mesh_tid(); f < nf; f += mesh_stride()) {
        if (!fkeep[f]) continue;
        const int32_t a = wf[3 * f], b = wf[3 * f + 1], c = wf[3 * f + 2];
        eslot[3 * f] = (unsigned int)edge_insert<true>(keys, cnt, own, mask, shift, a, b, (unsigned int)f);
        eslot[3 * f + 1] = (unsigned int)edge_insert<true>(keys, cnt, own, mask, shift, b, c, (unsigned int)f);
        eslot[3 * f + 2] = (unsigned int)edge_insert<true>(keys, cnt, own, mask, shift, c, a, (unsigned int)f);
    }
}

// one phase of the two largest keys (q, face) per slot with more than two owners; the planes a phase reads were
// finished by the launches before it
__global__ void __launch_bounds__(kMeshThreads)
k_rep_edge_rank(long long n_corners, const uint8_t* __restrict__ fkeep, const unsigned int* __restrict__ eslot,
                const unsigned int* __restrict__ cnt, const unsigned long long* __restrict__ qb, int phase,
                unsigned long long* m1q, int32_t* m1f, unsigned long long* m2q, int32_t* m2f)
{
    for (long long c = mesh_tid(); c < n_corners; c += mesh_stride()) {
        const long long f = c / 3;
        if (!fkeep[f]) continue;
        const unsigned int s = eslot[c];
        if (cnt[s] <= 2u) continue;
        const unsigned long long q = qb[f];
        if (phase == 0) {
            atomicMax(&m1q[s], q);
        } else if (phase == 1) {
            if (q == m1q[s]) atomicMax(&m1f[s], (int32_t)f);
        } else if (m1f[s] != (int32_t)f) {
            if (phase == 2) atomicMax(&m2q[s], q);
            else if (q == m2q[s]) atomicMax(&m2f[s], (int32_t)f);
        }
    }
}

// counts[rep_num_removed] += the faces that go (only with `act`); link[c] = c << 1 for every corner
__global__ void __launch_bounds__(kMeshThreads)
k_rep_face_remove(long long nf_padded, long long nf, const unsigned int* __restrict__ eslot,
                  const unsigned int* __restrict__ cnt, const int32_t* __restrict__ m1f, const int32_t* __restrict__ m2f,
                  int act, uint8_t* __restrict__ fkeep, unsigned int* __restrict__ link,
                  unsigned long long* __restrict__ counts)
{
    for (long long f = mesh_tid(); f < nf_padded; f += mesh_stride()) {
        bool gone = false;
        if (f < nf) {
            for (int k = 0; k < 3; ++k) link[3 * f + k] = (unsigned int)(3 * f + k) << 1;
            if (act && fkeep[f]) {
                for (int k = 0; k < 3; ++k) {
                    const unsigned int s = eslot[3 * f + k];
                    gone = gone || (cnt[s] > 2u && m1f[s] != (int32_t)f && m2f[s] != (int32_t)f);
                }
                if (gone) fkeep[f] = 0;
            }
        }
        wave_count(gone, &counts[rep_num_removed]);
    }
}

static __device__ __forceinline__ unsigned int rep_corner(const int32_t* __restrict__ wf, unsigned int f, int32_t x)
{
    const long long b = 3 * (long long)f;
    return (unsigned int)b + (wf[b] == x ? 0u : (wf[b + 1] == x ? 1u : 2u));
}

__global__ void __launch_bounds__(kMeshThreads)
k_rep_hook(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ cnt,
           const unsigned int* __restrict__ own, unsigned long long cap, const int32_t* __restrict__ wf,
           unsigned int* __restrict__ link)
{
    for (unsigned long long s = (unsigned long long)mesh_tid(); s < cap; s += (unsigned long long)mesh_stride()) {
        const unsigned long long key = keys[s];
        if (key == kEdgeEmpty || cnt[s] != 2u) continue;
        const unsigned int fa = own[2 * s] >> 1, fb = own[2 * s + 1] >> 1;
        const int32_t u = (int32_t)edge_lo(key), w = (int32_t)edge_hi(key);
        uf_union(link, rep_corner(wf, fa, u), rep_corner(wf, fb, u), 0u);
        uf_union(link, rep_corner(wf, fa, w), rep_corner(wf, fb, w), 0u);
    }
}

// wmin[w], wmax[w]: the smallest and the largest root among the corners of INPUT vertex w; mixed[r] = 1 where the set of
// root r holds corners of more than one input vertex
__global__ void __launch_bounds__(kMeshThreads)
k_rep_vertex_min(long long n_corners, const uint8_t* __restrict__ fkeep, const int32_t* __restrict__ face,
                 const int32_t* __restrict__ wf, const unsigned int* __restrict__ link, unsigned int* __restrict__ vmin,
                 uint8_t* __restrict__ ref, unsigned int* __restrict__ wmin, unsigned int* __restrict__ wmax,
                 uint8_t* __restrict__ mixed)
{
    for (long long c = mesh_tid(); c < n_corners; c += mesh_stride()) {
        if (!fkeep[c / 3]) continue;
        const int32_t x = wf[c], w = face[c];
        const unsigned int root = link[c] >> 1;
        atomicMin(&vmin[x], root);
        ref[x] = 1;
        atomicMin(&wmin[w], root);
        atomicMax(&wmax[w], root);
        if (face[root] != w) mixed[root] = 1;
    }
}

// a live root c that is not its vertex's minimum: where its set is exactly the corners of one welded input vertex w, the
// weld of w is undone (cback[c], vback[w]); else it opens a new vertex (isnew[c] with `split`, vsplit[x])
__global__ void __launch_bounds__(kMeshThreads)
k_rep_open(long long n_corners, const uint8_t* __restrict__ fkeep, const int32_t* __restrict__ face,
           const int32_t* __restrict__ wf, const unsigned int* __restrict__ link, const unsigned int* __restrict__ vmin,
           const unsigned int* __restrict__ wmin, const unsigned int* __restrict__ wmax, const uint8_t* __restrict__ mixed,
           int split, uint8_t* __restrict__ isnew, uint8_t* __restrict__ cback, uint8_t* __restrict__ vsplit,
           uint8_t* __restrict__ vback)
{
    for (long long c = mesh_tid(); c < n_corners; c += mesh_stride()) {
        bool extra = false, back = false;
        if (fkeep[c / 3]) {
            const int32_t x = wf[c], w = face[c];
            extra = (link[c] >> 1) == (unsigned int)c && vmin[x] != (unsigned int)c;
            back = extra && w != x && !mixed[c] && wmin[w] == (unsigned int)c && wmax[w] == (unsigned int)c;
            if (back) vback[w] = 1;
            else if (extra) vsplit[x] = 1;
        }
        isnew[c] = extra && !back && split;
        cback[c] = back;
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_rep_vertex_keep(long long nv_padded, long long nv, const int32_t* __restrict__ rep, const uint8_t* __restrict__ ref,
                  int drop, const uint8_t* __restrict__ vsplit, const uint8_t* __restrict__ vback,
                  uint8_t* __restrict__ vkeep, unsigned long long* __restrict__ counts)
{
    for (long long i = mesh_tid(); i < nv_padded; i += mesh_stride()) {
        bool dropped = false, is_split = false, back = false;
        if (i < nv) {
            back = vback[i] != 0;                                      // its weld is undone: it has corners
            const bool survivor = rep[i] == (int32_t)i;
            dropped = survivor && drop && !ref[i];
            vkeep[i] = (survivor && !dropped) || back;
            is_split = vsplit[i] != 0;
        }
        wave_count(dropped, &counts[rep_num_unreferenced]);
        wave_count(is_split, &counts[rep_num_split]);
        wave_count(back, &counts[rep_num_unwelded]);
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_rep_out_vertices(const double* __restrict__ v, long long nv, const int32_t* __restrict__ rep,
                   const int32_t* __restrict__ vidx, double* __restrict__ out_v, int32_t* __restrict__ origin,
                   int32_t* __restrict__ target)
{
    for (long long i = mesh_tid(); i < nv; i += mesh_stride()) {
        const int32_t t = vidx[i];
        if (t >= 0) {
            out_v[3 * (long long)t] = v[3 * i]; out_v[3 * (long long)t + 1] = v[3 * i + 1]; out_v[3 * (long long)t + 2] = v[3 * i + 2];
            origin[t] = (int32_t)i;
        }
        target[i] = t >= 0 ? t : vidx[rep[i]];
    }
}

// kv: the vertices k_rep_out_vertices wrote; new vertex cidx[root] follows them
__global__ void __launch_bounds__(kMeshThreads)
k_rep_out_corners(long long n_corners, const uint8_t* __restrict__ fkeep, const int32_t* __restrict__ fidx,
                  const int32_t* __restrict__ face, const int32_t* __restrict__ wf, const unsigned int* __restrict__ link,
                  const uint8_t* __restrict__ cback, const int32_t* __restrict__ vidx,
                  const int32_t* __restrict__ cidx, long long kv, const double* __restrict__ v,
                  int32_t* __restrict__ out_f, double* __restrict__ out_v, int32_t* __restrict__ origin)
{
    for (long long c = mesh_tid(); c < n_corners; c += mesh_stride()) {
        const long long f = c / 3;
        if (!fkeep[f]) continue;
        const int32_t x = wf[c];
        const unsigned int root = link[c] >> 1;
        const int32_t fresh = cidx[root];
        out_f[3 * (long long)fidx[f] + (c - 3 * f)] = fresh >= 0 ? (int32_t)(kv + fresh) : vidx[cback[root] ? face[root] : x];
        if (fresh >= 0 && root == (unsigned int)c) {
            const long long t = kv + fresh;
            out_v[3 * t] = v[3 * (long long)x]; out_v[3 * t + 1] = v[3 * (long long)x + 1]; out_v[3 * t + 2] = v[3 * (long long)x + 2];
            origin[t] = x;
        }
    }
}

hipError_t launch_rep_vertices(const double* v, long long nv, int weld, int32_t* table, int log2_cap, int32_t* rep,
                               unsigned long long* counts, hipStream_t s)
{
    const unsigned long long cap = 1ull << log2_cap;
    hipError_t he;
    if ((he = hipMemsetAsync(table, 0xFF, cap * 4, s)) != hipSuccess) return he;
    MESH_LAUNCH(k_rep_vertex_insert, mesh_grid(nv), v, nv, table, cap - 1, 64 - log2_cap, rep);
    MESH_LAUNCH(k_rep_vertex_rep, mesh_grid(nv), mesh_pad(nv), nv, table, weld, rep, counts);
    return hipSuccess;
}

hipError_t launch_rep_faces(const int32_t* face, long long nf, const int32_t* rep, const double* v, int drop_null,
                            int drop_copies, int32_t* table, int log2_cap, int32_t* wf, unsigned long long* qb,
                            int32_t* frep, uint8_t* fkeep, unsigned long long* counts, hipStream_t s)
{
    const unsigned long long cap = 1ull << log2_cap;
    hipError_t he;
    if ((he = hipMemsetAsync(table, 0xFF, cap * 4, s)) != hipSuccess) return he;
    MESH_LAUNCH(k_rep_face_classify, mesh_grid(nf), face, mesh_pad(nf), nf, rep, v, drop_null, table, cap - 1, 64 - log2_cap,
                wf, qb, frep, counts);
    MESH_LAUNCH(k_rep_face_rep, mesh_grid(nf), mesh_pad(nf), nf, table, frep, drop_copies, fkeep, counts);
    return hipSuccess;
}

hipError_t launch_rep_edges(const int32_t* wf, long long nf, const uint8_t* fkeep, unsigned long long* keys,
                            unsigned int* cnt, unsigned int* own, int log2_cap, unsigned int* eslot, hipStream_t s)
{
    const unsigned long long cap = 1ull << log2_cap;
    hipError_t he;
    if ((he = hipMemsetAsync(keys, 0xFF, cap * 8, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(cnt, 0, cap * 4, s)) != hipSuccess) return he;
    MESH_LAUNCH(k_rep_edge_insert, mesh_grid(nf), wf, nf, fkeep, keys, cnt, own, cap - 1, 64 - log2_cap, eslot);
    return hipSuccess;
}

hipError_t launch_rep_remove(long long nf, uint8_t* fkeep, const unsigned int* eslot, const unsigned int* cnt,
                             const unsigned long long* qb, int log2_cap, int act, unsigned long long* m1q, int32_t* m1f,
                             unsigned long long* m2q, int32_t* m2f, unsigned int* link, unsigned long long* counts,
                             hipStream_t s)
{
    const unsigned long long cap = 1ull << log2_cap;
    hipError_t he;
    if ((he = hipMemsetAsync(m1q, 0, cap * 8, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(m2q, 0, cap * 8, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(m1f, 0xFF, cap * 4, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(m2f, 0xFF, cap * 4, s)) != hipSuccess) return he;
    for (int phase = 0; phase < 4; ++phase)
        MESH_LAUNCH(k_rep_edge_rank, mesh_grid(3 * nf), 3 * nf, fkeep, eslot, cnt, qb, phase, m1q, m1f, m2q, m2f);
    MESH_LAUNCH(k_rep_face_remove, mesh_grid(nf), mesh_pad(nf), nf, eslot, cnt, m1f, m2f, act, fkeep, link, counts);
    return hipSuccess;
}

hipError_t launch_rep_hook(const unsigned long long* keys, const unsigned int* cnt, const unsigned int* own, int log2_cap,
                           const int32_t* wf, unsigned int* link, hipStream_t s)
{
    const unsigned long long cap = 1ull << log2_cap;
    MESH_LAUNCH(k_rep_hook, mesh_grid((long long)cap), keys, cnt, own, cap, wf, link);
    return hipSuccess;
}

hipError_t launch_rep_split(long long nf, long long nv, const uint8_t* fkeep, const int32_t* face, const int32_t* wf,
                            const unsigned int* link, const int32_t* rep, int split, int drop, unsigned int* vmin,
                            unsigned int* wmin, unsigned int* wmax, uint8_t* ref, uint8_t* vsplit, uint8_t* vback,
                            uint8_t* mixed, uint8_t* isnew, uint8_t* cback, uint8_t* vkeep, unsigned long long* counts,
                            hipStream_t s)
{
    hipError_t he;
    if ((he = hipMemsetAsync(vmin, 0xFF, (size_t)nv * 4, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(wmin, 0xFF, (size_t)nv * 4, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(wmax, 0, (size_t)nv * 4, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(ref, 0, (size_t)nv, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(vsplit, 0, (size_t)nv, s)) != hipSuccess) return he;
    if ((he = hipMemsetAsync(vback, 0, (size_t)nv, s)) != hipSuccess) return he;
    if (nf > 0 && (he = hipMemsetAsync(mixed, 0, (size_t)(3 * nf), s)) != hipSuccess) return he;
    MESH_LAUNCH(k_rep_vertex_min, mesh_grid(3 * nf), 3 * nf, fkeep, face, wf, link, vmin, ref, wmin, wmax, mixed);
    MESH_LAUNCH(k_rep_open, mesh_grid(3 * nf), 3 * nf, fkeep, face, wf, link, vmin, wmin, wmax, mixed, split, isnew, cback,
                vsplit, vback);
    MESH_LAUNCH(k_rep_vertex_keep, mesh_grid(nv), mesh_pad(nv), nv, rep, ref, drop, vsplit, vback, vkeep, counts);
    return hipSuccess;
}

hipError_t launch_rep_output(const double* v, long long nv, const int32_t* rep, const int32_t* vidx, long long nf,
                             const uint8_t* fkeep, const int32_t* fidx, const int32_t* face, const int32_t* wf,
                             const unsigned int* link, const uint8_t* cback, const int32_t* cidx, long long kv, double* out_v, int32_t* out_f, int32_t* origin,
                             int32_t* target, hipStream_t s)
{
    MESH_LAUNCH(k_rep_out_vertices, mesh_grid(nv), v, nv, rep, vidx, out_v, origin, target);
    MESH_LAUNCH(k_rep_out_corners, mesh_grid(3 * nf), 3 * nf, fkeep, fidx, face, wf, link, cback, vidx, cidx, kv, v, out_f, out_v,
                origin);
    return hipSuccess;
}

}  // namespace mm
