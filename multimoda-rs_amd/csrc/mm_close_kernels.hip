// mm_close_kernels.hip -- the data-parallel part of the CCTA mesh closing, for gfx950: the open half-edges of a mesh
// read off the assembly's edge table, the fans that close its holes, and the labelling's label smoothing.
//
// manual_hole_fill (multimodars/ccta/fixing_functions.py:13-49) and smooth_mesh_labels
// (src/ccta/binding/ccta_py.rs:743-814).  include/mm_ccta.h states the rules; every stage has an exact, order-free
// answer, so the output does not depend on scheduling.  The edge table is that of mm_mesh_device.h as
// mm_weld_kernels.hip fills it; the winding and the volume are those of mm_weld_kernels.hip.
//
//   k_close_half_edges   one lane per slot of the edge table: a slot owned by exactly one face gives the half-edge
//                        a -> b as that face traverses it (with the flip of the winding stage where it ran), packed
//                        a << 32 | b.  A wave takes its room in the list with one atomicAdd of its ballot's count;
//                        the order of the list is therefore not fixed, and the host's walk does not depend on it.
//   k_close_fan          face nf + i = (b_i, a_i, nv + loop_i) from the walk-ordered fan list the host uploads.
//   k_smooth_vote        one lane per face.  vote[v] is one word per vertex: 0 = no neighbour seen, L + 1 = every
//                        neighbour seen so far carries L, kSmoothMixed = two labels seen.  The word only ever moves
//                        0 -> L + 1 -> mixed, so a lane first reads it (a relaxed device-scope load: a stale value is
//                        an earlier state and at worst costs a redundant atomic) and touches it with an atomic only
//                        where it has to move: in a smooth region that is one atomicCAS per vertex and reads
//                        otherwise, against twelve min / max atomics per face for a pair of min and max words.
//   k_smooth_apply       one lane per vertex: next[v] = L where vote[v] == L + 1 and L != cur[v], else cur[v]; the word
//                        is cleared for the next iteration; flips counted per wave.
//   k_smooth_csr         one lane per vertex over its row of a CSR adjacency: the same rule in one launch.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mm_device.h"
#include "mm_mesh_device.h"

namespace mm {

static constexpr unsigned int kSmoothMixed = 0x7FFFFFFFu;

// cap is a multiple of kMeshThreads: every lane of a wave runs the same number of rounds (the ballots need it)
__global__ void __launch_bounds__(kMeshThreads)
k_close_half_edges(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ cnt,
                   const unsigned int* __restrict__ own, unsigned long long cap, const unsigned int* __restrict__ link,
                   unsigned long long* __restrict__ out, unsigned long long out_cap, unsigned long long* __restrict__ n_out)
{
    for (unsigned long long s = (unsigned long long)mesh_tid(); s < cap; s += (unsigned long long)mesh_stride()) {
        const unsigned long long key = keys[s];
        const bool open = key != kEdgeEmpty && cnt[s] == 1u;
        unsigned long long he = 0;
        if (open) {
            const unsigned int o = own[2 * s];
            const unsigned int dir = (o ^ (link ? link[o >> 1] : 0u)) & 1u;      // 1: from the smaller to the larger end
            he = dir ? key : (((unsigned long long)edge_hi(key) << 32) | edge_lo(key));
        }
        const unsigned long long at = wave_append(open, n_out);
        if (open && at < out_cap) out[at] = he;                                   // never beyond: open edges <= 3 nf
    }
}

// fan[3 i .. 3 i + 2] = (a, b, loop) of the i-th half-edge of the loops in walk order
__global__ void __launch_bounds__(kMeshThreads)
k_close_fan(const int32_t* __restrict__ fan, long long n_fan, int32_t nv, int32_t* __restrict__ face, long long nf)
{
    for (long long i = mesh_tid(); i < n_fan; i += mesh_stride()) {
        int32_t* f = face + 3 * (nf + i);
        f[0] = fan[3 * i + 1];
        f[1] = fan[3 * i];
        f[2] = nv + fan[3 * i + 2];
    }
}

static __device__ __forceinline__ void smooth_mixed(unsigned int* __restrict__ w)
{
    if (__atomic_load_n(w, __ATOMIC_RELAXED) != kSmoothMixed) atomicMax(w, kSmoothMixed);
}

// a neighbour with label l (0 .. 255) votes at the word w
static __device__ __forceinline__ void smooth_vote(unsigned int* __restrict__ w, unsigned int l)
{
    const unsigned int mine = l + 1u;
    unsigned int seen = __atomic_load_n(w, __ATOMIC_RELAXED);
    if (seen == 0u) seen = atomicCAS(w, 0u, mine);
    if (seen == 0u || seen == mine || seen == kSmoothMixed) return;
    atomicMax(w, kSmoothMixed);
}

__global__ void __launch_bounds__(kMeshThreads)
k_smooth_vote(const int32_t* __restrict__ face, long long nf, const uint8_t* __restrict__ cur, unsigned int* __restrict__ vote)
{
    for (long long f = mesh_tid(); f < nf; f += mesh_stride()) {
        const int32_t a = face[3 * f], b = face[3 * f + 1], c = face[3 * f + 2];
        const unsigned int la = cur[a], lb = cur[b], lc = cur[c];
        if (lb == lc) smooth_vote(&vote[a], lb); else smooth_mixed(&vote[a]);
        if (la == lc) smooth_vote(&vote[b], la); else smooth_mixed(&vote[b]);
        if (la == lb) smooth_vote(&vote[c], la); else smooth_mixed(&vote[c]);
    }
}

// nv_padded is a multiple of the workgroup; *n_flips += the vertices that changed (one atomicAdd per wave)
__global__ void __launch_bounds__(kMeshThreads)
k_smooth_apply(long long nv_padded, long long nv, const uint8_t* __restrict__ cur, unsigned int* __restrict__ vote,
               uint8_t* __restrict__ next, unsigned long long* __restrict__ n_flips)
{
    for (long long v = mesh_tid(); v < nv_padded; v += mesh_stride()) {
        bool flip = false;
        if (v < nv) {
            const unsigned int w = vote[v];
            const uint8_t own = cur[v];
            flip = w != 0u && w != kSmoothMixed && (uint8_t)(w - 1u) != own;
            next[v] = flip ? (uint8_t)(w - 1u) : own;
            if (w != 0u) vote[v] = 0u;
        }
        wave_count(flip, n_flips);
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_smooth_csr(long long nv_padded, long long nv, const int32_t* __restrict__ off, const int32_t* __restrict__ nb,
             const uint8_t* __restrict__ cur, uint8_t* __restrict__ next, unsigned long long* __restrict__ n_flips)
{
    for (long long v = mesh_tid(); v < nv_padded; v += mesh_stride()) {
        bool flip = false;
        if (v < nv) {
            const int32_t lo = off[v], hi = off[v + 1];
            const uint8_t own = cur[v];
            uint8_t to = own;
            if (hi > lo) {
                to = cur[nb[lo]];
                bool same = true;
                for (int32_t k = lo + 1; k < hi && same; ++k) same = cur[nb[k]] == to;
                if (!same) to = own;
            }
            flip = to != own;
            next[v] = to;
        }
        wave_count(flip, n_flips);
    }
}

hipError_t launch_close_half_edges(const unsigned long long* keys, const unsigned int* cnt, const unsigned int* own,
                                   int log2_cap, const unsigned int* link, unsigned long long* out,
                                   unsigned long long out_cap, unsigned long long* n_out, hipStream_t s)
{
    const unsigned long long cap = 1ull << log2_cap;                   // at least kMeshThreads (the host sizes it)
    hipError_t he;
    if ((he = hipMemsetAsync(n_out, 0, 8, s)) != hipSuccess) return he;
    MESH_LAUNCH(k_close_half_edges, mesh_grid((long long)cap), keys, cnt, own, cap, link, out, out_cap, n_out);
    return hipSuccess;
}

hipError_t launch_close_fan(const int32_t* fan, long long n_fan, long long nv, int32_t* face, long long nf, hipStream_t s)
{
    if (n_fan > 0) MESH_LAUNCH(k_close_fan, mesh_grid(n_fan), fan, n_fan, (int32_t)nv, face, nf);
    return hipSuccess;
}

hipError_t launch_smooth_faces(const int32_t* face, long long nf, long long nv, const uint8_t* cur, unsigned int* vote,
                               uint8_t* next, unsigned long long* n_flips, int* launches, hipStream_t s)
{
    if (nf > 0) {
        MESH_LAUNCH(k_smooth_vote, mesh_grid(nf), face, nf, cur, vote);
        ++*launches;
    }
    MESH_LAUNCH(k_smooth_apply, mesh_grid(nv), mesh_pad(nv), nv, cur, vote, next, n_flips);
    ++*launches;
    return hipSuccess;
}

hipError_t launch_smooth_csr(const int32_t* off, const int32_t* nb, long long nv, const uint8_t* cur, uint8_t* next,
                             unsigned long long* n_flips, int* launches, hipStream_t s)
{
    MESH_LAUNCH(k_smooth_csr, mesh_grid(nv), mesh_pad(nv), nv, off, nb, cur, next, n_flips);
    ++*launches;
    return hipSuccess;
}

}  // namespace mm
