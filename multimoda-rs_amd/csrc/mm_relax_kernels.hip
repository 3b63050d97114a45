// mm_relax_kernels.hip -- CCTA mesh relaxation for gfx950 (include/mm_ccta.h, "mesh relaxation"): tangential Jacobi steps
// whose every candidate is put back on a reference surface by the exact point-to-triangle search of mm_tri_kernels.hip.
// The mesh, the reference's staged faces, the queries (the free vertices in slab order) and the (query block, chunk)
// items stay on the device from step 0 to the last iteration; the host launches and reads nothing in between.
//
//   k_relax_accept       step 0, one lane per query: the closest point becomes the vertex's position, the winner's key its
//                        face; vq[vertex] = the query; the largest d2 by an integer atomicMax on the bits, one per wave.
//   k_relax_candidates   one workgroup per query block (the block of k_tri_min's items), one lane per query: the row's
//                        neighbours in row order, acc = acc + w * x_j unfused as k_smooth_step sums them, the tangential
//                        part of acc - x against the normal of the query's face, the candidate c = x + lambda t.  The
//                        query's new minimum is seeded with face_d2(c, that face) -- the inlined function k_tri_min folds
//                        over (mm_tri_device.h), so the seed is a member of the set and every item may run checked.  Then
//                        the block's box of candidates (min / max through shuffles and LDS: exact, any order) and, one
//                        lane per item of the block, the refreshed lb2 = box_lb2(block box, chunk box, tri_slack): the
//                        functions of mm_prune.h the host built step 0's bounds with.
//   k_relax_guard        one lane per mesh face: the normal before the iteration against the normal behind it; a face that
//                        would turn marks its free corners (atomicOr).
//   k_relax_apply        one lane per query: an unmarked query takes its closest point and winner, a marked one keeps
//                        both and is counted (ballot, one atomicAdd per wave).
//   k_relax_flipped      one lane per mesh face: input normal against final normal, counted the same way.
// Integer atomics only; no floating-point atomics, no assembly.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mm_device.h"
#include "mm_mesh_device.h"
#include "mm_prune.h"
#include "mm_prune_device.h"
#include "mm_tri_device.h"

namespace mm {

static constexpr unsigned long long kNoFace = ~0ull;
enum : unsigned int { kRelaxStays = 1u, kRelaxGuarded = 2u };          // bits of a query's state

static __device__ __forceinline__ void store3(double* p, long long i, const V3& v)
{
    p[3 * i] = v.x; p[3 * i + 1] = v.y; p[3 * i + 2] = v.z;
}

static __device__ __forceinline__ unsigned long long wave_max(unsigned long long m)
{
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned long long other = (unsigned long long)__shfl_xor((long long)m, s);
        m = other > m ? other : m;
    }
    return m;
}

__global__ void __launch_bounds__(kMeshThreads)
k_relax_accept(const int32_t* __restrict__ qv, long long nq_padded, long long nq, const double* __restrict__ closest,
               const unsigned long long* __restrict__ key, const unsigned long long* __restrict__ sq,
               double* __restrict__ x, unsigned long long* __restrict__ fkey, int32_t* __restrict__ vq,
               unsigned long long* __restrict__ num)
{
    for (long long j = mesh_tid(); j < nq_padded; j += mesh_stride()) {
        unsigned long long m = 0ull;
        if (j < nq) {
            const int32_t v = qv[j];
            const unsigned long long k = key[j];
            fkey[j] = k;
            vq[v] = (int32_t)j;
            if (k != kNoFace) {                                          // no face beat anything: the vertex stays
                store3(x, v, load3(closest, j));
                m = sq[j];
            }
        }
        m = wave_max(m);
        if (__lane_id() == 0 && m) atomicMax(&num[relax_num_init], m);
    }
}

// grid = the query blocks; qpb = queries per block, ch = faces per chunk, per = the block's items of pass B
__global__ void __launch_bounds__(kMeshThreads)
k_relax_candidates(const int32_t* __restrict__ off, const int32_t* __restrict__ nb, const double* __restrict__ x,
                   const int32_t* __restrict__ qv, int nq, const unsigned long long* __restrict__ fkey,
                   const double4* __restrict__ tri, double lambda, double* __restrict__ qxyz,
                   unsigned long long* __restrict__ sq, unsigned long long* __restrict__ key,
                   unsigned int* __restrict__ state, TriWork* __restrict__ work, int n_a, int per, int qpb, int ch,
                   const Box3* __restrict__ cbox)
{
    __shared__ double s_box[kMeshThreads / 64][6];
    const int tid = threadIdx.x, b = blockIdx.x;
    const int q0 = b * qpb, q1 = q0 + qpb < nq ? q0 + qpb : nq;
    Box3 box;
    for (int q = q0 + tid; q < q1; q += kMeshThreads) {
        const long long v = qv[q];
        const V3 p = load3(x, v);
        const int32_t r0 = off[v], r1 = off[v + 1];
        const double w = 1.0 / (double)(r1 - r0);                       // a free vertex has a neighbour
        V3 acc{0.0, 0.0, 0.0};
        for (int32_t k = r0; k < r1; ++k) {
            const double* pj = x + 3 * (long long)nb[k];
            acc.x = acc.x + w * pj[0];
            acc.y = acc.y + w * pj[1];
            acc.z = acc.z + w * pj[2];
        }
        const V3 d = sub3(acc, p);
        const unsigned long long fk = fkey[q];
        bool stays = fk == kNoFace;
        V3 cand = p;
        V3 fa{}, fb{}, fc{};
        int kind = kFaceProper;
        if (!stays) {
            const long long j = (long long)(fk & 0xffffffffull);
            const double4 ta = tri[3 * j], tb = tri[3 * j + 1], tc = tri[3 * j + 2];
            fa = V3{ta.x, ta.y, ta.z}; fb = V3{tb.x, tb.y, tb.z}; fc = V3{tc.x, tc.y, tc.z};
            kind = (int)__double_as_longlong(ta.w);
            const V3 n = cross3(sub3(fb, fa), sub3(fc, fa));
            const double nn = dot3(n, n);
            V3 t = d;
            if (nn > 0.0 && nn < __builtin_inf()) {
                const double s = dot3(n, d) / nn;
                t = V3{d.x - n.x * s, d.y - n.y * s, d.z - n.z * s};
            }
            const V3 c{p.x + lambda * t.x, p.y + lambda * t.y, p.z + lambda * t.z};
            if (__builtin_isfinite(c.x) && __builtin_isfinite(c.y) && __builtin_isfinite(c.z)) cand = c;
            else stays = true;
        }
        unsigned long long seed = kInfBits;
        if (fk != kNoFace) {
            const double d2 = face_d2(cand, fa, fb, fc, sub3(fb, fa), sub3(fc, fa), kind);
            if (d2 == d2) seed = (unsigned long long)__double_as_longlong(d2);
        }
        store3(qxyz, q, cand);
        sq[q] = seed;
        key[q] = kNoFace;
        state[q] = stays ? kRelaxStays : 0u;
        const double c3[3] = {cand.x, cand.y, cand.z};
        box.add(c3);
    }
    // the block's box: min and max are exact, so the order of the merge does not show
    for (int a = 0; a < 3; ++a) {
        for (int s = 1; s < 64; s <<= 1) {
            const double lo = __shfl_xor(box.lo[a], s), hi = __shfl_xor(box.hi[a], s);
            box.lo[a] = lo < box.lo[a] ? lo : box.lo[a];
            box.hi[a] = hi > box.hi[a] ? hi : box.hi[a];
        }
    }
    if (__lane_id() == 0)
        for (int a = 0; a < 3; ++a) { s_box[tid >> 6][a] = box.lo[a]; s_box[tid >> 6][3 + a] = box.hi[a]; }
    __syncthreads();
    for (int wv = 0; wv < kMeshThreads / 64; ++wv)
        for (int a = 0; a < 3; ++a) {
            const double lo = s_box[wv][a], hi = s_box[wv][3 + a];
            box.lo[a] = lo < box.lo[a] ? lo : box.lo[a];
            box.hi[a] = hi > box.hi[a] ? hi : box.hi[a];
        }
    // one lane per item of the block: item 0 is the block's item of pass A, the others its run of pass B
    for (int i = tid; i <= per; i += kMeshThreads) {
        const long long at = i == 0 ? (long long)b : (long long)n_a + (long long)b * per + (i - 1);
        const Box3 cb = cbox[work[at].c0 / ch];
        work[at].lb2 = box_lb2(box, cb, tri_slack(box, cb));
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_relax_guard(const int32_t* __restrict__ face, long long nf, const double* __restrict__ x,
              const double* __restrict__ closest, const unsigned long long* __restrict__ key,
              const int32_t* __restrict__ vq, unsigned int* __restrict__ state)
{
    for (long long f = mesh_tid(); f < nf; f += mesh_stride()) {
        const int32_t c[3] = {face[3 * f], face[3 * f + 1], face[3 * f + 2]};
        if (c[0] == c[1] || c[1] == c[2] || c[0] == c[2]) continue;
        V3 o[3], n[3];
        int32_t q[3];
        for (int k = 0; k < 3; ++k) {
            o[k] = load3(x, c[k]);
            q[k] = vq[c[k]];
            const bool moves = q[k] >= 0 && !(__atomic_load_n(&state[q[k]], __ATOMIC_RELAXED) & kRelaxStays) &&
                               key[q[k]] != kNoFace;
            n[k] = moves ? load3(closest, q[k]) : o[k];
        }
        const V3 m_old = cross3(sub3(o[1], o[0]), sub3(o[2], o[0]));
        const V3 m_new = cross3(sub3(n[1], n[0]), sub3(n[2], n[0]));
        if (dot3(m_old, m_old) > 0.0 && !(dot3(m_old, m_new) > 0.0))
            for (int k = 0; k < 3; ++k)
                if (q[k] >= 0) atomicOr(&state[q[k]], kRelaxGuarded);
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_relax_apply(const int32_t* __restrict__ qv, long long nq_padded, long long nq, const double* __restrict__ closest,
              const unsigned long long* __restrict__ key, const unsigned int* __restrict__ state, double* __restrict__ x,
              unsigned long long* __restrict__ fkey, unsigned long long* __restrict__ num)
{
    for (long long j = mesh_tid(); j < nq_padded; j += mesh_stride()) {
        const bool reverted = j < nq && (state[j] != 0u || key[j] == kNoFace);
        if (j < nq && !reverted) {
            store3(x, qv[j], load3(closest, j));
            fkey[j] = key[j];
        }
        wave_count(reverted, &num[relax_num_reverted]);
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_relax_flipped(const int32_t* __restrict__ face, long long nf_padded, long long nf, const double* __restrict__ v0,
                const double* __restrict__ x, unsigned long long* __restrict__ num)
{
    for (long long f = mesh_tid(); f < nf_padded; f += mesh_stride()) {
        bool flipped = false;
        if (f < nf) {
            const int32_t a = face[3 * f], b = face[3 * f + 1], c = face[3 * f + 2];
            if (a != b && b != c && a != c) {
                const V3 ia = load3(v0, a), xa = load3(x, a);
                const V3 m_in = cross3(sub3(load3(v0, b), ia), sub3(load3(v0, c), ia));
                const V3 m_out = cross3(sub3(load3(x, b), xa), sub3(load3(x, c), xa));
                flipped = dot3(m_in, m_in) > 0.0 && dot3(m_in, m_out) <= 0.0;
            }
        }
        wave_count(flipped, &num[relax_num_flipped]);
    }
}

hipError_t launch_relax_accept(const int32_t* qv, int nq, const double* closest, const unsigned long long* key,
                               const unsigned long long* sq, double* x, unsigned long long* fkey, int32_t* vq,
                               unsigned long long* num, hipStream_t s)
{
    MESH_LAUNCH(k_relax_accept, mesh_grid(nq), qv, mesh_pad(nq), (long long)nq, closest, key, sq, x, fkey, vq, num);
    return hipSuccess;
}

hipError_t launch_relax_candidates(const int32_t* off, const int32_t* nb, const double* x, const int32_t* qv, int nq,
                                   const unsigned long long* fkey, const double* tri12, double lambda, double* qxyz,
                                   unsigned long long* sq, unsigned long long* key, unsigned int* state, TriWork* work,
                                   int n_a, int n_b, const double* cbox, hipStream_t s)
{
    if (nq <= 0 || n_a <= 0 || n_b % n_a != 0) return hipErrorInvalidValue;
    MESH_LAUNCH(k_relax_candidates, (unsigned)n_a, off, nb, x, qv, nq, fkey, (const double4*)tri12, lambda, qxyz, sq, key,
                state, work, n_a, n_b / n_a, tri_queries_per_block(), tri_chunk_faces(), (const Box3*)cbox);
    return hipSuccess;
}

hipError_t launch_relax_guard(const int32_t* face, long long nf, const double* x, const double* closest,
                              const unsigned long long* key, const int32_t* vq, unsigned int* state, hipStream_t s)
{
    MESH_LAUNCH(k_relax_guard, mesh_grid(nf), face, nf, x, closest, key, vq, state);
    return hipSuccess;
}

hipError_t launch_relax_apply(const int32_t* qv, int nq, const double* closest, const unsigned long long* key,
                              const unsigned int* state, double* x, unsigned long long* fkey, unsigned long long* num,
                              hipStream_t s)
{
    MESH_LAUNCH(k_relax_apply, mesh_grid(nq), qv, mesh_pad(nq), (long long)nq, closest, key, state, x, fkey, num);
    return hipSuccess;
}

hipError_t launch_relax_flipped(const int32_t* face, long long nf, const double* v0, const double* x,
                                unsigned long long* num, hipStream_t s)
{
    MESH_LAUNCH(k_relax_flipped, mesh_grid(nf), face, mesh_pad(nf), nf, v0, x, num);
    return hipSuccess;
}

}  // namespace mm
