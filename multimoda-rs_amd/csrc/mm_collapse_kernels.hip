// mm_collapse_kernels.hip -- CCTA mesh edge collapse for gfx950: the collapse of an isotropic remesh
// (multimodars/ccta/fixing_functions.py:207-219, collapseflag), pass after pass, until no short edge may go.
//
// include/mm_ccta.h ("mesh edge collapse") states the rule, which has no visiting order: a half-edge collapse r -> k moves
// no surviving vertex, every guard is a "for all" over the ring of r, every candidate carries a priority that is unique in
// the mesh, and it collapses where that priority is the largest on the closed star of r, so the closed stars of the
// removed vertices are disjoint and the answer is one whatever the scheduling.  One lane per item in grid-stride loops;
// integer atomics only.  The ring of r is its row of the sorted adjacency (launch_mesh_csr of mm_smooth_kernels.hip, built
// from the same table); the faces at a removable r are, one per ring vertex n, the owner that traverses r -> n.
//
//   k_edge_insert_first (mm_mesh_device.h) the three edges of every live face into the edge table: the count, the first
//                      two owners with their direction bits, and the smallest corner id with an atomicMin.
//   k_col_valence      one lane per slot: deg (low 30 bits of a vertex word, atomicAdd), the border flag (bit 31) and the
//                      inconsistent flag (bit 30) with an atomicOr; the edges, the open, non-manifold, inconsistent and
//                      short ones by ballot; the mark of a short edge per slot.
//   k_col_candidates   one lane per slot: a short edge's guards in both directions, the choice, the counts by ballot, the
//                      priority and (r, k) per slot, a 64-bit atomicMax into best over the closed star of r.
//   k_col_apply        one lane per slot: a candidate that is best on its closed star puts k in the place of r in the faces
//                      at r, marks the two owners and r dead and leaves r -> k.
//   k_col_finish       one lane per vertex: the chain of r -> k followed to a survivor; origin and target.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mm_device.h"
#include "mm_mesh_device.h"
#include "mm_tri_device.h"

namespace mm {

static constexpr unsigned int kColBorder = 0x80000000u;
static constexpr unsigned int kColTwisted = 0x40000000u;
static constexpr unsigned int kColDeg = 0x3FFFFFFFu;

static __device__ __forceinline__ bool col_removable(unsigned int w, const uint8_t* __restrict__ pin, int32_t x)
{
    return (w & (kColBorder | kColTwisted)) == 0u && (w & kColDeg) >= 3u && !(pin && pin[x]);
}

// the face at r that traverses r -> n (r removable: the edge has two owners of opposite directions); -1 without the edge
static __device__ __forceinline__ long long col_face_at(const unsigned long long* __restrict__ keys,
                                                        const unsigned int* __restrict__ own, unsigned long long mask,
                                                        int shift, int32_t r, int32_t n)
{
    const unsigned long long s = edge_find(keys, mask, shift, r, n);
    if (s == kEdgeEmpty) return -1;
    const unsigned int o0 = own[2 * s], o1 = own[2 * s + 1];
    return (long long)((((o0 & 1u) != 0u) == (r < n) ? o0 : o1) >> 1);
}

// cap is a multiple of kMeshThreads, as is the stride
__global__ void __launch_bounds__(kMeshThreads)
k_col_valence(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ cnt,
              const unsigned int* __restrict__ own, unsigned long long cap, const double* __restrict__ v, double thr_min2,
              unsigned int* __restrict__ vw, unsigned long long* __restrict__ mark, unsigned long long* __restrict__ counts)
{
    for (unsigned long long s = (unsigned long long)mesh_tid(); s < cap; s += (unsigned long long)mesh_stride()) {
        const unsigned long long k = keys[s];
        const bool used = k != kEdgeEmpty;
        const unsigned int lo = edge_lo(k), hi = edge_hi(k);
        const bool edge = used && lo != hi;
        const unsigned int c = used ? cnt[s] : 0u;
        bool twisted = false, is_short = false;
        if (used && c == 2u) twisted = ((own[2 * s] ^ own[2 * s + 1]) & 1u) == 0u;
        if (edge) {
            atomicAdd(&vw[lo], 1u);
            atomicAdd(&vw[hi], 1u);
            is_short = len_sq3(load3(v, lo), load3(v, hi)) < thr_min2;
        }
        if (used && c != 2u) {
            atomicOr(&vw[lo], kColBorder);
            atomicOr(&vw[hi], kColBorder);
        }
        if (twisted) {                                                 // an (a, a) edge owned twice has both bits 0
            atomicOr(&vw[lo], kColTwisted);
            atomicOr(&vw[hi], kColTwisted);
        }
        wave_count(edge, &counts[col_num_edges]);
        wave_count(c == 1u, &counts[col_num_open]);
        wave_count(c > 2u, &counts[col_num_nonmanifold]);
        wave_count(edge && twisted, &counts[col_num_inconsistent]);
        wave_count(is_short, &counts[col_num_short]);
        mark[s] = is_short ? ((c == 2u && !twisted) ? 1ull : 2ull) : 0ull;   // 1: short and two owners of opposite directions
    }
}

// the guards (c) .. (g) of the collapse r -> k of an edge whose owners fp, fm have the opposite corners c, d: 0, or 1 .. 5
// for the first class that fails; *longest = the largest squared length of a new edge.  Every guard is a flag or an exact
// minimum / maximum over the ring, so the order of the row does not matter.
static __device__ __forceinline__ int col_direction(int32_t r, int32_t k, int32_t c, int32_t d, long long fp, long long fm,
                                                    const unsigned long long* __restrict__ keys,
                                                    const unsigned int* __restrict__ own, unsigned long long mask, int shift,
                                                    const int32_t* __restrict__ face, const double* __restrict__ v,
                                                    const unsigned int* __restrict__ vw, const int32_t* __restrict__ off,
                                                    const int32_t* __restrict__ nb, double thr_max2, double cc2, double qk2,
                                                    double* longest)
{
    const unsigned int wc = vw[c], wd = vw[d];
    const long long after_k = (long long)(vw[k] & kColDeg) + (long long)(vw[r] & kColDeg) - 4;
    const bool valence_ok = after_k >= 3 && (long long)(wc & kColDeg) - 1 >= ((wc & kColBorder) ? 2 : 3) &&
                            (long long)(wd & kColDeg) - 1 >= ((wd & kColBorder) ? 2 : 3);
    int common = 0;
    bool too_long = false, turned = false, nan = false;
    double lng = 0.0, q_new = __longlong_as_double(0x7FF0000000000000ll), t_old = q_new;
    for (int32_t i = off[r], e = off[r + 1]; i < e; ++i) {
        const int32_t n = nb[i];
        if (n != k && edge_find(keys, mask, shift, n, k) != kEdgeEmpty) ++common;
        if (n != k && n != c && n != d) {
            const double x = len_sq3(load3(v, k), load3(v, n));
            if (!(x <= thr_max2)) too_long = true;
            else if (x > lng) lng = x;
        }
        const long long f = col_face_at(keys, own, mask, shift, r, n);
        if (f < 0) continue;
        const int32_t a0 = face[3 * f], a1 = face[3 * f + 1], a2 = face[3 * f + 2];
        const int32_t x = a0 == r ? a1 : (a1 == r ? a2 : a0), y = a0 == r ? a2 : (a1 == r ? a0 : a1);
        const V3 pr = load3(v, r), px = load3(v, x), py = load3(v, y);
        const V3 n_old = cross3(sub3(px, pr), sub3(py, pr));
        const double t = qk2 * tri_quality(pr, px, py, n_old);
        nan = nan || t != t;
        t_old = t < t_old ? t : t_old;
        if (f == fp || f == fm) continue;
        const V3 pk = load3(v, k);
        const V3 n_new = cross3(sub3(px, pk), sub3(py, pk));
        const double dn = dot3(n_old, n_new);
        if (!(dn > 0.0 && dn * dn >= cc2 * (dot3(n_old, n_old) * dot3(n_new, n_new)))) turned = true;
        const double qn = tri_quality(pk, px, py, n_new);
        nan = nan || qn != qn;
        q_new = qn < q_new ? qn : q_new;
    }
    *longest = lng;
    if (common != 2) return 1;
    if (!valence_ok) return 2;
    if (too_long) return 3;
    if (turned) return 4;
    return (nan || !(q_new >= t_old)) ? 5 : 0;
}

__global__ void __launch_bounds__(kMeshThreads)
k_col_candidates(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ own, const unsigned int* __restrict__ first, unsigned long long cap,
                 int shift, const int32_t* __restrict__ face, const double* __restrict__ v,
                 const uint8_t* __restrict__ pin, const unsigned int* __restrict__ vw, const int32_t* __restrict__ off,
                 const int32_t* __restrict__ nb, double thr_max2, double cc2, double qk2,
                 unsigned long long* __restrict__ prio, int32_t* __restrict__ rk, unsigned long long* __restrict__ best,
                 unsigned long long* __restrict__ counts)
{
    for (unsigned long long s = (unsigned long long)mesh_tid(); s < cap; s += (unsigned long long)mesh_stride()) {
        const unsigned long long key = keys[s];
        const int32_t lo = (int32_t)edge_lo(key), hi = (int32_t)edge_hi(key);
        int reason = -1;                                               // -1: not short; 0: a candidate; 1 .. 5: (c) .. (g); 6: fixed
        int32_t r = 0, k = 0;
        const unsigned long long marked = prio[s];                     // k_col_valence: 0, or 1 / 2 at a short edge
        {
            if (marked != 0ull) {
                const bool rem_lo = col_removable(vw[lo], pin, lo), rem_hi = col_removable(vw[hi], pin, hi);
                const unsigned int o0 = own[2 * s], o1 = own[2 * s + 1];
                if (!rem_lo && !rem_hi) {
                    reason = 6;
                } else if (marked != 1ull) {                           // (a): the set bit runs lo -> hi
                    reason = 1;
                } else {
                    const long long fp = (long long)(((o0 & 1u) ? o0 : o1) >> 1), fm = (long long)(((o0 & 1u) ? o1 : o0) >> 1);
                    const int32_t p0 = face[3 * fp], p1 = face[3 * fp + 1], p2 = face[3 * fp + 2];
                    const int32_t m0 = face[3 * fm], m1 = face[3 * fm + 1], m2 = face[3 * fm + 2];
                    const bool distinct = p0 != p1 && p1 != p2 && p0 != p2 && m0 != m1 && m1 != m2 && m0 != m2;
                    const int32_t c = (p0 != lo && p0 != hi) ? p0 : ((p1 != lo && p1 != hi) ? p1 : p2);
                    const int32_t d = (m0 != lo && m0 != hi) ? m0 : ((m1 != lo && m1 != hi) ? m1 : m2);
                    if (!(distinct && c != d)) {
                        reason = 1;
                    } else {
                        int fail_hi = -1, fail_lo = -1;                // -1: (b) fails, the end is not removable
                        double long_hi = 0.0, long_lo = 0.0;
                        for (int t = 0; t < 2; ++t) {                  // r = hi, then r = lo
                            const int32_t rr = t ? lo : hi, kk = t ? hi : lo;
                            if (!(t ? rem_lo : rem_hi)) continue;
                            double lng;
                            const int fail = col_direction(rr, kk, c, d, fp, fm, keys, own, cap - 1, shift, face, v, vw, off,
                                                           nb, thr_max2, cc2, qk2, &lng);
                            if (t) { fail_lo = fail; long_lo = lng; }
                            else { fail_hi = fail; long_hi = lng; }
                        }
                        if (fail_hi != 0 && fail_lo != 0) {
                            reason = rem_hi ? fail_hi : fail_lo;
                        } else {
                            reason = 0;
                            r = (fail_hi == 0 && fail_lo == 0) ? (long_lo < long_hi ? lo : hi) : (fail_hi == 0 ? hi : lo);
                            k = r == lo ? hi : lo;
                        }
                    }
                }
            }
        }
        unsigned long long p = 0;
        if (reason == 0) {
            const double l2 = len_sq3(load3(v, lo), load3(v, hi));
            const unsigned long long top = 0xFFFFFFFFull - ((unsigned long long)__double_as_longlong(l2) >> 32);
            p = (top << 32) | (unsigned long long)(0xFFFFFFFFu - first[s]);
            rk[2 * s] = r;
            rk[2 * s + 1] = k;
            atomicMax(&best[r], p);
            for (int32_t i = off[r], e = off[r + 1]; i < e; ++i) atomicMax(&best[nb[i]], p);
        }
        prio[s] = p;
        wave_count(reason == 0, &counts[col_num_candidates]);
        wave_count(reason == 6, &counts[col_num_fixed]);
        wave_count(reason == 1, &counts[col_num_link]);
        wave_count(reason == 2, &counts[col_num_valence]);
        wave_count(reason == 3, &counts[col_num_long]);
        wave_count(reason == 4, &counts[col_num_normal]);
        wave_count(reason == 5, &counts[col_num_quality]);
    }
}

// The closed stars of the winners are disjoint: no face that one of them rewrites is read or written by another.
__global__ void __launch_bounds__(kMeshThreads)
k_col_apply(const unsigned long long* __restrict__ keys, const unsigned int* __restrict__ own, unsigned long long cap,
            int shift, const unsigned long long* __restrict__ prio, const int32_t* __restrict__ rk,
            const unsigned long long* __restrict__ best, const int32_t* __restrict__ off, const int32_t* __restrict__ nb,
            int32_t* __restrict__ face, uint8_t* __restrict__ fkeep, uint8_t* __restrict__ vkeep, int32_t* __restrict__ to,
            unsigned long long* __restrict__ counts)
{
    for (unsigned long long s = (unsigned long long)mesh_tid(); s < cap; s += (unsigned long long)mesh_stride()) {
        const unsigned long long p = prio[s];
        bool wins = false;
        if (p != 0ull) {
            const int32_t r = rk[2 * s], k = rk[2 * s + 1];
            const int32_t b = off[r], e = off[r + 1];
            wins = best[r] == p;
            for (int32_t i = b; i < e && wins; ++i) wins = best[nb[i]] == p;
            if (wins) {
                const long long f0 = (long long)(own[2 * s] >> 1), f1 = (long long)(own[2 * s + 1] >> 1);
                for (int32_t i = b; i < e; ++i) {
                    const long long f = col_face_at(keys, own, cap - 1, shift, r, nb[i]);
                    if (f < 0 || f == f0 || f == f1) continue;
                    int32_t* a = face + 3 * f;
                    if (a[0] == r) a[0] = k;
                    else if (a[1] == r) a[1] = k;
                    else if (a[2] == r) a[2] = k;
                }
                fkeep[f0] = 0;
                fkeep[f1] = 0;
                vkeep[r] = 0;
                to[r] = k;
            }
        }
        wave_count(wins, &counts[col_num_collapses]);
    }
}

// to: -1 at a survivor, else the vertex it collapsed into; a chain has at most one link a pass
__global__ void __launch_bounds__(kMeshThreads)
k_col_finish(const int32_t* __restrict__ to, const int32_t* __restrict__ vidx, long long nv, int32_t* __restrict__ origin,
             int32_t* __restrict__ target)
{
    for (long long x = mesh_tid(); x < nv; x += mesh_stride()) {
        long long t = x;
        for (int32_t next = to[t]; next >= 0; next = to[t]) t = next;
        target[x] = vidx[t];
        if (t == x) origin[vidx[x]] = (int32_t)x;
    }
}

// the edge table, the vertex words and counts[edges .. short] of the live faces as they are; counts[0 .. col_num_pass)
// cleared
hipError_t launch_col_table(const int32_t* face, long long nf, const uint8_t* fkeep, long long nv, const double* v,
                            double thr_min2, unsigned long long* keys, unsigned int* cnt, unsigned int* own,
                            unsigned int* first, int log2_cap, unsigned int* vw, unsigned long long* prio,
                            unsigned long long* counts, hipStream_t s)
{
    const unsigned long long cap = 1ull << log2_cap;                   // at least kMeshThreads (the host sizes it)
    const hipError_t he = edge_first_clear(keys, cnt, first, cap, vw, nv, counts, col_num_pass, s);
    if (he != hipSuccess) return he;
    MESH_LAUNCH(k_edge_insert_first<true>, mesh_grid(nf), face, nf, fkeep, keys, cnt, own, first, cap - 1, 64 - log2_cap);
    MESH_LAUNCH(k_col_valence, mesh_grid((long long)cap), keys, cnt, own, cap, v, thr_min2, vw, prio, counts);
    return hipSuccess;
}

// behind launch_col_table and launch_mesh_csr on the same keys: the candidates of the pass, then the collapses, in place
hipError_t launch_col_pass(int32_t* face, long long nv, const double* v, const uint8_t* pin, const unsigned long long* keys,
                           const unsigned int* own, const unsigned int* first, int log2_cap, const unsigned int* vw,
                           const int32_t* off, const int32_t* nb, double thr_max2, double cc2, double qk2, unsigned long long* prio, int32_t* rk, unsigned long long* best,
                           uint8_t* fkeep, uint8_t* vkeep, int32_t* to, unsigned long long* counts, hipStream_t s)
{
    const unsigned long long cap = 1ull << log2_cap;
    const hipError_t he = hipMemsetAsync(best, 0, (size_t)nv * 8, s);
    if (he != hipSuccess) return he;
    MESH_LAUNCH(k_col_candidates, mesh_grid((long long)cap), keys, own, first, cap, 64 - log2_cap, face, v, pin, vw, off,
                nb, thr_max2, cc2, qk2, prio, rk, best, counts);
    MESH_LAUNCH(k_col_apply, mesh_grid((long long)cap), keys, own, cap, 64 - log2_cap, prio, rk, best, off, nb, face, fkeep,
                vkeep, to, counts);
    return hipSuccess;
}

hipError_t launch_col_finish(const int32_t* to, const int32_t* vidx, long long nv, int32_t* origin, int32_t* target,
                             hipStream_t s)
{
    MESH_LAUNCH(k_col_finish, mesh_grid(nv), to, vidx, nv, origin, target);
    return hipSuccess;
}

}  // namespace mm
