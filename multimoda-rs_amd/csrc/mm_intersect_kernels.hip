// mm_intersect_kernels.hip -- triangle-triangle intersection states in 3-D, f64, for gfx950: the mesh intersection check
// of include/mm_ccta.h ("mesh intersections").  Every pair of faces that reaches the narrow phase gets the state of
// mm_isect_device.h: a pure function of the two faces, every operation unfused and in the header's order (the file is
// built with -ffp-contract=off), so the chunking, the order of the items and the culling cannot change a bit.
//
// Mapping: one work item = a chunk I of 256 faces against a chunk J whose closed boxes overlap (the host culls the
// others: faces of chunks with disjoint boxes have disjoint boxes and are disjoint by the box step).  One workgroup of
// 256 lanes per item.  A lane keeps one face of chunk I in registers: nine doubles, its box, three canonical ids and
// its original index.  Chunk J sits in LDS as three double4 per face (24 KiB), ids and index in the w words; all lanes
// read the same address (a broadcast, conflict-free) and the ids are made scalar with readfirstlane.  Per (lane, face
// of J): the box step, 6 min/max and 6 compares; the few survivors run the narrow phase under divergence (about 30 to
// 200 f64 operations).  In an I == I item the lane whose staged position is below the other's handles the pair.
//
// Outputs: per-face flags by atomicOr into the byte of the face's staged position in a cleared word array; integer
// atomicAdd counters; the pairs through an atomicAdd cursor into a buffer of `cap` records, dropped beyond it -- the
// host sorts them, so their order here does not matter.  k_isect_clear clears flags and counters on every call.
#include <hip/hip_runtime.h>

#include "mm_device.h"
#include "mm_isect_device.h"

namespace mm {

static constexpr int kIsectChunk = 256;   // 256 faces x 3 double4 = 24 KiB of LDS

__device__ __forceinline__ unsigned long long isect_scalar_bits(double w)
{
    const unsigned long long v = (unsigned long long)__double_as_longlong(w);
    const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)v);
    const unsigned int hi = __builtin_amdgcn_readfirstlane((unsigned int)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

__device__ __forceinline__ double min3(double a, double b, double c) { return __builtin_fmin(__builtin_fmin(a, b), c); }
__device__ __forceinline__ double max3(double a, double b, double c) { return __builtin_fmax(__builtin_fmax(a, b), c); }

__global__ void __launch_bounds__(256)
k_isect_clear(unsigned int* __restrict__ state, long long n_words, unsigned long long* __restrict__ counters)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n_words) state[i] = 0u;
    if (i < 8) counters[i] = 0ull;
}

template <bool SELF>
__global__ void __launch_bounds__(256)
k_isect_pairs(const int2* __restrict__ items, int n_items, const double4* __restrict__ tri, int n_a, int n_b, int off_b,
              unsigned int* __restrict__ state, unsigned long long* __restrict__ counters,
              unsigned long long* __restrict__ pairs, unsigned long long cap)
{
    using namespace isect;
    constexpr int CH = kIsectChunk;
    __shared__ double4 s_t[3 * CH];
    __shared__ unsigned int s_narrow;
    const int tid = threadIdx.x;
    for (int wi = blockIdx.x; wi < n_items; wi += gridDim.x) {
        const int2 it = items[wi];
        const int i = it.x * CH + tid;
        const int ic = i < n_a ? i : n_a - 1;                         // lanes past the end hold the last face and an empty box
        const double4 la = tri[3 * (long long)ic], lb = tri[3 * (long long)ic + 1], lc = tri[3 * (long long)ic + 2];
        const P3 p{la.x, la.y, la.z}, q{lb.x, lb.y, lb.z}, r{lc.x, lc.y, lc.z};
        const unsigned long long wa = (unsigned long long)__double_as_longlong(la.w);
        const unsigned long long wb = (unsigned long long)__double_as_longlong(lb.w);
        const int id_p = (int)(unsigned int)wa, id_q = (int)(wa >> 32), id_r = (int)(unsigned int)wb;
        const int orig = (int)(wb >> 32);
        const bool live = i < n_a && __double_as_longlong(lc.w) == 0;
        // an empty box overlaps nothing: lanes past the end and degenerate faces test against nothing
        const double lox = live ? min3(p.x, q.x, r.x) : 1.7976931348623157e308, hix = live ? max3(p.x, q.x, r.x) : -1.7976931348623157e308;
        const double loy = min3(p.y, q.y, r.y), hiy = max3(p.y, q.y, r.y);
        const double loz = min3(p.z, q.z, r.z), hiz = max3(p.z, q.z, r.z);
        const int c0 = it.y * CH;
        const int n = n_b - c0 < CH ? n_b - c0 : CH;
        const bool diagonal = SELF && it.x == it.y;
        __syncthreads();   // previous chunk fully consumed, previous count read
        for (int j = tid; j < 3 * n; j += 256) s_t[j] = tri[3 * ((long long)off_b + c0) + j];
        if (tid == 0) s_narrow = 0u;
        __syncthreads();
        unsigned int narrow = 0u;
        for (int j = 0; j < n; ++j) {
            const double4 ta = s_t[3 * j], tb = s_t[3 * j + 1], tc = s_t[3 * j + 2];
            if (isect_scalar_bits(tc.w) != 0ull) continue;            // a degenerate face: uniform
            bool hit = live && min3(ta.x, tb.x, tc.x) <= hix && max3(ta.x, tb.x, tc.x) >= lox &&
                       min3(ta.y, tb.y, tc.y) <= hiy && max3(ta.y, tb.y, tc.y) >= loy &&
                       min3(ta.z, tb.z, tc.z) <= hiz && max3(ta.z, tb.z, tc.z) >= loz;
            if (diagonal) hit = hit && tid < j;
            if (!hit) continue;
            ++narrow;
            const unsigned long long ua = isect_scalar_bits(ta.w), ub = isect_scalar_bits(tb.w);
            const int jd_p = (int)(unsigned int)ua, jd_q = (int)(ua >> 32), jd_r = (int)(unsigned int)ub;
            const int jorig = (int)(ub >> 32);
            const P3 jp{ta.x, ta.y, ta.z}, jq{tb.x, tb.y, tb.z}, jr{tc.x, tc.y, tc.z};
            // face 1 of the rule: the lower original index (self form), the first mesh's face (two-mesh form)
            const bool first = SELF ? orig < jorig : true;
            const int st = SELF ? pair_state(pick(first, p, jp), pick(first, q, jq), pick(first, r, jr), first ? id_p : jd_p,
                                             first ? id_q : jd_q, first ? id_r : jd_r, pick(first, jp, p), pick(first, jq, q),
                                             pick(first, jr, r), first ? jd_p : id_p, first ? jd_q : id_q, first ? jd_r : id_r)
                                : pair_state(p, q, r, 0, 1, 2, jp, jq, jr, 3, 4, 5);
            if (st == kDisjoint) continue;
            const unsigned int bits = (unsigned int)st & 3u;
            const long long pos_l = i, pos_j = (long long)off_b + c0 + j;
            atomicOr(&state[pos_l >> 2], bits << (8 * (int)(pos_l & 3)));
            atomicOr(&state[pos_j >> 2], bits << (8 * (int)(pos_j & 3)));
            atomicAdd(&counters[bits == 1u ? 0 : 1], 1ull);
            if (st & kCoincident) atomicAdd(&counters[2], 1ull);
            const unsigned long long slot = atomicAdd(&counters[4], 1ull);
            if (slot < cap) {
                const unsigned long long lo = (unsigned long long)(first ? orig : jorig), hi = (unsigned long long)(first ? jorig : orig);
                pairs[slot] = ((unsigned long long)bits << 62) | (lo << 31) | hi;
            }
        }
        if (narrow) atomicAdd(&s_narrow, narrow);
        __syncthreads();
        if (tid == 0 && s_narrow) atomicAdd(&counters[3], (unsigned long long)s_narrow);
    }
}

int isect_chunk_faces() { return kIsectChunk; }
int isect_launches() { return 2; }

hipError_t launch_isect_pairs(const int32_t* items, int n_items, const double* tri12, int n_a, int n_b, int off_b,
                              bool self_form, unsigned int* state, long long n_state_words, unsigned long long* counters,
                              unsigned long long* pairs, unsigned long long cap, hipStream_t s)
{
    if (n_items <= 0 || n_a <= 0 || n_b <= 0 || n_state_words <= 0) return hipErrorInvalidValue;
    const long long clear = n_state_words > 8 ? n_state_words : 8;
    hipLaunchKernelGGL(k_isect_clear, dim3((unsigned)((clear + 255) / 256)), dim3(256), 0, s, state, n_state_words, counters);
    const dim3 grid((unsigned)(n_items < (1 << 20) ? n_items : (1 << 20)));
    const double4* tri = (const double4*)tri12;
    if (self_form)
        hipLaunchKernelGGL((k_isect_pairs<true>), grid, dim3(256), 0, s, (const int2*)items, n_items, tri, n_a, n_b, off_b,
                           state, counters, pairs, cap);
    else
        hipLaunchKernelGGL((k_isect_pairs<false>), grid, dim3(256), 0, s, (const int2*)items, n_items, tri, n_a, n_b, off_b,
                           state, counters, pairs, cap);
    return hipGetLastError();
}

}  // namespace mm
