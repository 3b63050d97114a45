// mm_flip_kernels.hip -- CCTA mesh edge flips for gfx950: the swap of an isotropic remesh
// (multimodars/ccta/fixing_functions.py:207-219, swapflag), pass after pass, until no flip lowers the valence deviation.
//
// include/mm_ccta.h ("mesh edge flips") states the rule, which has no visiting order: every candidate edge carries a
// priority that is unique in the mesh, and it flips where that priority is the largest at all four of its vertices, so
// flipped edges share no vertex and the answer is one whatever the scheduling.  One lane per item in grid-stride loops;
// integer atomics only.
//
//   k_edge_insert_first (mm_mesh_device.h) the three edges of every face into the edge table: the count, the first two
//                       owners with their direction bits, and the smallest corner id with an atomicMin.
//   k_flip_valence      one lane per slot: deg (low 31 bits of a vertex word, atomicAdd) and the border flag (bit 31,
//                       atomicOr); the edges, the open, non-manifold, inconsistent and masked ones by ballot.
//   k_flip_deviation    one lane per vertex: the sum of (deg - target)^2, one atomicAdd per wave.
//   k_flip_candidates   one lane per slot: the tests (a) .. (h), the counts by ballot, the priority and the two opposite
//                       corners per slot, a 64-bit atomicMax into best at the four vertices.
//   k_flip_apply        one lane per slot: a candidate that is best at its four vertices rewrites its two faces.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mm_device.h"
#include "mm_mesh_device.h"
#include "mm_tri_device.h"

namespace mm {

static constexpr unsigned int kFlipBorder = 0x80000000u;

// deg - (border ? 4 : 6) of a vertex word
static __device__ __forceinline__ long long flip_excess(unsigned int w)
{
    return (long long)(w & ~kFlipBorder) - ((w & kFlipBorder) ? 4 : 6);
}

// cap is a multiple of kMeshThreads, as is the stride
__global__ void __launch_bounds__(kMeshThreads)
k_flip_valence(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ cnt,
               const unsigned int* __restrict__ own, unsigned long long cap, const uint8_t* __restrict__ pin,
               unsigned int* __restrict__ vw, unsigned long long* __restrict__ counts)
{
    for (unsigned long long s = (unsigned long long)mesh_tid(); s < cap; s += (unsigned long long)mesh_stride()) {
        const unsigned long long k = keys[s];
        const bool used = k != kEdgeEmpty;
        const unsigned int lo = edge_lo(k), hi = edge_hi(k);
        const bool edge = used && lo != hi;
        const unsigned int c = used ? cnt[s] : 0u;
        bool twisted = false, masked = false;
        if (edge) {
            atomicAdd(&vw[lo], 1u);
            atomicAdd(&vw[hi], 1u);
            if (c == 2u) twisted = ((own[2 * s] ^ own[2 * s + 1]) & 1u) == 0u;
            if (pin) masked = (pin[lo] | pin[hi]) != 0;
        }
        if (used && c != 2u) {
            atomicOr(&vw[lo], kFlipBorder);
            atomicOr(&vw[hi], kFlipBorder);
        }
        wave_count(edge, &counts[flip_num_edges]);
        wave_count(c == 1u, &counts[flip_num_open]);
        wave_count(c > 2u, &counts[flip_num_nonmanifold]);
        wave_count(twisted, &counts[flip_num_inconsistent]);
        wave_count(masked, &counts[flip_num_masked]);
    }
}

// n_pad: nv up to a multiple of kMeshThreads
__global__ void __launch_bounds__(kMeshThreads)
k_flip_deviation(const unsigned int* __restrict__ vw, long long nv, long long n_pad, unsigned long long* __restrict__ counts)
{
    for (long long v = mesh_tid(); v < n_pad; v += mesh_stride()) {
        long long x = 0;
        if (v < nv) {
            const long long ex = flip_excess(vw[v]);
            x = ex * ex;
        }
        for (int d = 1; d < 64; d <<= 1) x += __shfl_xor(x, d);
        if (__lane_id() == 0 && x) atomicAdd(&counts[flip_num_deviation], (unsigned long long)x);
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_flip_candidates(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ cnt,
                  const unsigned int* __restrict__ own, const unsigned int* __restrict__ first, unsigned long long cap,
                  int shift, const int32_t* __restrict__ face, const double* __restrict__ v,
                  const uint8_t* __restrict__ pin, const unsigned int* __restrict__ vw, double cc2, double qk2,
                  unsigned long long* __restrict__ prio, int32_t* __restrict__ opp, unsigned long long* __restrict__ best,
                  unsigned long long* __restrict__ counts)
{
    for (unsigned long long s = (unsigned long long)mesh_tid(); s < cap; s += (unsigned long long)mesh_stride()) {
        const unsigned long long k = keys[s];
        const int32_t lo = (int32_t)edge_lo(k), hi = (int32_t)edge_hi(k);
        int32_t c = 0, d = 0;
        long long g = 0;
        bool open = false;                                             // (a) .. (d) hold
        if (k != kEdgeEmpty && lo != hi && cnt[s] == 2u) {
            const unsigned int o0 = own[2 * s], o1 = own[2 * s + 1];
            if ((o0 ^ o1) & 1u) {                                      // (a): the set bit runs lo -> hi
                const long long fp = (long long)(((o0 & 1u) ? o0 : o1) >> 1), fm = (long long)(((o0 & 1u) ? o1 : o0) >> 1);
                const int32_t p0 = face[3 * fp], p1 = face[3 * fp + 1], p2 = face[3 * fp + 2];
                const int32_t m0 = face[3 * fm], m1 = face[3 * fm + 1], m2 = face[3 * fm + 2];
                const bool distinct = p0 != p1 && p1 != p2 && p0 != p2 && m0 != m1 && m1 != m2 && m0 != m2;
                c = (p0 != lo && p0 != hi) ? p0 : ((p1 != lo && p1 != hi) ? p1 : p2);
                d = (m0 != lo && m0 != hi) ? m0 : ((m1 != lo && m1 != hi) ? m1 : m2);
                const bool free_ends = !pin || (pin[lo] | pin[hi]) == 0;
                if (distinct && c != d && free_ends) {                 // (b), (c)
                    g = 2 * (flip_excess(vw[lo]) + flip_excess(vw[hi]) - flip_excess(vw[c]) - flip_excess(vw[d])) - 4;
                    open = g > 0;                                      // (d)
                }
            }
        }
        int blocked = 0;                                               // 1 .. 4: the guard (e) .. (h) that failed
        if (open) {
            if (edge_find(keys, cap - 1, shift, c, d) != kEdgeEmpty) {
                blocked = 1;
            } else {
                const V3 pl = load3(v, lo), ph = load3(v, hi), pc = load3(v, c), pd = load3(v, d);
                const V3 n0 = cross3(sub3(ph, pl), sub3(pc, pl));
                const V3 n1 = cross3(sub3(pl, ph), sub3(pd, ph));
                const V3 m0 = cross3(sub3(pd, pl), sub3(pc, pl));
                const V3 m1 = cross3(sub3(pc, ph), sub3(pd, ph));
                const double dn = dot3(n0, n1);
                if (!(dot3(m0, n0) > 0.0 && dot3(m0, n1) > 0.0 && dot3(m1, n0) > 0.0 && dot3(m1, n1) > 0.0)) {
                    blocked = 2;
                } else if (!(dn > 0.0 && dn * dn >= cc2 * (dot3(n0, n0) * dot3(n1, n1)))) {
                    blocked = 3;
                } else {
                    const double t0 = qk2 * tri_quality(pl, ph, pc, n0), t1 = qk2 * tri_quality(ph, pl, pd, n1);
                    const double q0 = tri_quality(pl, pd, pc, m0), q1 = tri_quality(ph, pc, pd, m1);
                    if (!(q0 >= t0 && q0 >= t1 && q1 >= t0 && q1 >= t1)) blocked = 4;
                }
            }
        }
        const bool cand = open && blocked == 0;
        unsigned long long p = 0;
        if (cand) {
            p = ((unsigned long long)(g < (1ll << 20) ? g : (1ll << 20)) << 32) | (unsigned long long)(0xFFFFFFFFu - first[s]);
            opp[2 * s] = c;
            opp[2 * s + 1] = d;
            atomicMax(&best[lo], p);
            atomicMax(&best[hi], p);
            atomicMax(&best[c], p);
            atomicMax(&best[d], p);
        }
        prio[s] = p;
        wave_count(cand, &counts[flip_num_candidates]);
        wave_count(blocked == 1, &counts[flip_num_existing]);
        wave_count(blocked == 2, &counts[flip_num_normal]);
        wave_count(blocked == 3, &counts[flip_num_crease]);
        wave_count(blocked == 4, &counts[flip_num_quality]);
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_flip_apply(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ own, unsigned long long cap,
             const unsigned long long* __restrict__ prio, const int32_t* __restrict__ opp,
             const unsigned long long* __restrict__ best, int32_t* __restrict__ face, unsigned long long* __restrict__ counts)
{
    for (unsigned long long s = (unsigned long long)mesh_tid(); s < cap; s += (unsigned long long)mesh_stride()) {
        const unsigned long long p = prio[s];
        bool flips = false;
        if (p != 0ull) {
            const unsigned long long k = keys[s];
            const int32_t lo = (int32_t)edge_lo(k), hi = (int32_t)edge_hi(k), c = opp[2 * s], d = opp[2 * s + 1];
            flips = best[lo] == p && best[hi] == p && best[c] == p && best[d] == p;
            if (flips) {
                const unsigned int o0 = own[2 * s], o1 = own[2 * s + 1];
                int32_t* fp = face + 3 * (long long)(((o0 & 1u) ? o0 : o1) >> 1);
                int32_t* fm = face + 3 * (long long)(((o0 & 1u) ? o1 : o0) >> 1);
                fp[0] = lo; fp[1] = d; fp[2] = c;
                fm[0] = hi; fm[1] = c; fm[2] = d;
            }
        }
        wave_count(flips, &counts[flip_num_flips]);
    }
}

// the edge table and the vertex words of the faces as they are; counts[0 .. flip_num_pass) cleared
hipError_t launch_flip_valence(const int32_t* face, long long nf, long long nv, const uint8_t* pin,
                               unsigned long long* keys, unsigned int* cnt, unsigned int* own, unsigned int* first,
                               int log2_cap, unsigned int* vw, unsigned long long* counts, hipStream_t s)
{
    const unsigned long long cap = 1ull << log2_cap;                   // at least kMeshThreads (the host sizes it)
    const hipError_t he = edge_first_clear(keys, cnt, first, cap, vw, nv, counts, flip_num_pass, s);
    if (he != hipSuccess) return he;
    MESH_LAUNCH(k_edge_insert_first<false>, mesh_grid(nf), face, nf, (const uint8_t*)nullptr, keys, cnt, own, first, cap - 1,
                64 - log2_cap);
    MESH_LAUNCH(k_flip_valence, mesh_grid((long long)cap), keys, cnt, own, cap, pin, vw, counts);
    MESH_LAUNCH(k_flip_deviation, mesh_grid(nv), vw, nv, mesh_pad(nv), counts);
    return hipSuccess;
}

// behind launch_flip_valence: the candidates of the pass, then the flips, in place
hipError_t launch_flip_pass(int32_t* face, long long nv, const double* v, const uint8_t* pin, const unsigned long long* keys,
                            const unsigned int* cnt, const unsigned int* own, const unsigned int* first, int log2_cap,
                            const unsigned int* vw, double cc2, double qk2, unsigned long long* prio, int32_t* opp,
                            unsigned long long* best, unsigned long long* counts, hipStream_t s)
{
    const unsigned long long cap = 1ull << log2_cap;
    const hipError_t he = hipMemsetAsync(best, 0, (size_t)nv * 8, s);
    if (he != hipSuccess) return he;
    MESH_LAUNCH(k_flip_candidates, mesh_grid((long long)cap), keys, cnt, own, first, cap, 64 - log2_cap, face, v, pin, vw, cc2,
                qk2, prio, opp, best, counts);
    MESH_LAUNCH(k_flip_apply, mesh_grid((long long)cap), keys, own, cap, prio, opp, best, face, counts);
    return hipSuccess;
}

}  // namespace mm
