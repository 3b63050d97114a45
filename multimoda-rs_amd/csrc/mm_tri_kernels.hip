// mm_tri_kernels.hip -- exact point-to-triangle squared distances in 3-D, f64, for gfx950: the surface distance of
// include/mm_ccta.h ("surface distance").  For every query p:  out[p] = min_f d2(p, face f), with d2 the squared distance
// to Ericson's closest point (Real-Time Collision Detection 5.1.5), every operation unfused and in the header's order
// (the file is built with -ffp-contract=off), every quotient a true division.  min is exact, so the result does not
// depend on the traversal order.
//
// Mapping: one work item = 256 lanes x QPT queries against one chunk of CH faces; a chunk is staged in LDS as three
// double4 per face (corner a, b, c), so that a corner is two ds_read broadcasts (all lanes read the same address:
// conflict-free).  a.w carries the bits of the face's kind (0 proper, 1 degenerate, 2 thin), b.w those of its original
// index; both are the same for all lanes and are made scalar with readfirstlane, so the branch on the kind is uniform.
// Per (query, face): 9 sub, 6 dots (30), 3 cross terms (9), then the branch of the query's region -- a vertex (nothing),
// an edge (1 division, 3 mul-add pairs) or the interior (2 divisions, 6 pairs) -- and the squared distance (8): about 60
// fp64 VALU operations and at most 2 divisions against 6/QPT LDS reads -> fp64-VALU bound.  The divisions stay inside
// their branches: lanes of other regions are masked off while they run.
//
// Pruning (mm_prune.h, mm_prune_device.h): pass A is k_tri_min<.., false, false>, pass B <.., true, false>,
// which counts the items it skips.  Particular to this kernel is the winner: the who pass (<.., false, true>) takes, over
// the items whose bound does not exceed the block's largest final minimum, the lowest original face index whose d2 equals
// the query's final minimum, by the same merge on (original index << 32 | staged position); k_tri_closest then
// recomputes closest point and region of that face, one lane per query.
#include <hip/hip_runtime.h>

#include "mm_device.h"
#include "mm_prune_device.h"
#include "mm_tri_device.h"
#include "mm_xcd.h"

namespace mm {

static constexpr int kTriChunk = 256;   // 256 faces x 3 double4 = 24 KiB of LDS: 6 blocks a CU by LDS
static constexpr int kTriQpt = 2;

__device__ __forceinline__ unsigned long long scalar_bits(double w)
{
    const unsigned long long v = (unsigned long long)__double_as_longlong(w);
    const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)v);
    const unsigned int hi = __builtin_amdgcn_readfirstlane((unsigned int)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// sq, key: nq entries each; counters[0]: the items pass B skips
__global__ void __launch_bounds__(256)
k_tri_fill(unsigned long long* __restrict__ sq, unsigned long long* __restrict__ key, long long nq,
           unsigned long long* __restrict__ counters)
{
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < nq) { sq[i] = kInfBits; key[i] = ~0ull; }
    if (i == 0) counters[0] = 0ull;
}

// WHO = false: the minima (CHECK: pass B).  WHO = true: the winners' keys, from the final minima in sq.
template <int QPT, bool CHECK, bool WHO>
__global__ void __launch_bounds__(256)
k_tri_min(const TriWork* __restrict__ work, int n_work, const double4* __restrict__ tri, int nf,
          const double* __restrict__ qxyz, int nq, unsigned long long* __restrict__ sq,
          unsigned long long* __restrict__ key, unsigned long long* __restrict__ counters)
{
    constexpr int NT = 256, CH = kTriChunk;
    __shared__ double4 s_t[3 * CH];
    __shared__ unsigned long long s_max;
    const int tid = threadIdx.x;
    for (int wi = (int)gridDim.x == n_work ? xcd_work_index(blockIdx.x, n_work) : (int)blockIdx.x; wi < n_work;
         wi += gridDim.x) {
        const TriWork w = work[wi];
        double fin[QPT];   // WHO: the final minimum to match (NaN where the query has none)
        if (CHECK || WHO) {
            // largest current minimum of this block's queries (a stale, larger value only costs work)
            unsigned long long mx = 0ull;
#pragma unroll
            for (int k = 0; k < QPT; ++k) {
                const int q = w.q0 + k * NT + tid;
                const unsigned long long v = q < nq ? sq[q] : 0ull;
                mx = v > mx ? v : mx;
                fin[k] = q < nq && v != kInfBits ? __longlong_as_double((long long)v) : __builtin_nan("");
            }
            const double top = __longlong_as_double((long long)block_max(mx, &s_max));
            if (skip_item(WHO ? Skip::cannot_equal : Skip::cannot_lower, w.lb2, top)) {   // uniform
                if (CHECK && tid == 0) atomicAdd(&counters[0], 1ull);
                continue;
            }
        }
        V3 p[QPT];
        double m[QPT];
        unsigned long long best[QPT];
#pragma unroll
        for (int k = 0; k < QPT; ++k) {
            const int q = w.q0 + k * NT + tid;
            const int qc = q < nq ? q : nq - 1;   // lanes past the end recompute the last query, never stored
            p[k] = V3{qxyz[3 * (long long)qc], qxyz[3 * (long long)qc + 1], qxyz[3 * (long long)qc + 2]};
            m[k] = __builtin_inf();
            best[k] = ~0ull;
        }
        const int n = nf - w.c0 < CH ? nf - w.c0 : CH;
        __syncthreads();   // previous chunk fully consumed
        for (int j = tid; j < 3 * n; j += NT) s_t[j] = tri[3 * (long long)w.c0 + j];
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const double4 ta = s_t[3 * j], tb = s_t[3 * j + 1], tc = s_t[3 * j + 2];
            const V3 a{ta.x, ta.y, ta.z}, b{tb.x, tb.y, tb.z}, c{tc.x, tc.y, tc.z};
            const V3 ab = sub3(b, a), ac = sub3(c, a);
            const int kind = (int)scalar_bits(ta.w);   // uniform: proper, degenerate or thin
            const unsigned long long id = WHO ? (scalar_bits(tb.w) << 32) | (unsigned int)(w.c0 + j) : 0ull;
#pragma unroll
            for (int k = 0; k < QPT; ++k) {
                const double v = face_d2(p[k], a, b, c, ab, ac, kind);
                if (WHO) best[k] = v == fin[k] && id < best[k] ? id : best[k];
                else m[k] = v < m[k] ? v : m[k];
            }
        }
#pragma unroll
        for (int k = 0; k < QPT; ++k) {
            const int q = w.q0 + k * NT + tid;
            if (q >= nq) continue;
            if (WHO) merge_min(&key[q], best[k]);
            else merge_min(&sq[q], (unsigned long long)__double_as_longlong(m[k]));
        }
    }
}

// one lane per query: closest point and region of the winner (key >> 32 = its original index, the low word its staged
// position); a query without a winner gets NaN and -1
__global__ void __launch_bounds__(256)
k_tri_closest(const double4* __restrict__ tri, const double* __restrict__ qxyz, int nq,
              const unsigned long long* __restrict__ key, double* __restrict__ closest, int32_t* __restrict__ region)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    const unsigned long long k = key[q];
    V3 c{__builtin_nan(""), __builtin_nan(""), __builtin_nan("")};
    int r = -1;
    if (k != ~0ull) {
        const long long j = (long long)(k & 0xffffffffull);
        const double4 ta = tri[3 * j], tb = tri[3 * j + 1], tc = tri[3 * j + 2];
        const V3 a{ta.x, ta.y, ta.z}, b{tb.x, tb.y, tb.z}, cc{tc.x, tc.y, tc.z};
        const V3 p{qxyz[3 * (long long)q], qxyz[3 * (long long)q + 1], qxyz[3 * (long long)q + 2]};
        c = face_closest(p, a, b, cc, sub3(b, a), sub3(cc, a), (int)__double_as_longlong(ta.w), r);
    }
    closest[3 * (long long)q] = c.x; closest[3 * (long long)q + 1] = c.y; closest[3 * (long long)q + 2] = c.z;
    region[q] = r;
}

int tri_queries_per_block() { return 256 * kTriQpt; }
int tri_chunk_faces() { return kTriChunk; }

// work: n_a items of pass A, then n_b of pass B; the who pass runs over all of them.  Launches: tri_launches(n_b).
hipError_t launch_tri_distance(const TriWork* work, int n_a, int n_b, const double* tri12, int nf, const double* qxyz, int nq,
                               unsigned long long* sq, unsigned long long* key, double* closest, int32_t* region,
                               unsigned long long* counters, hipStream_t s)
{
    if (nq <= 0 || nf <= 0 || n_a <= 0) return hipErrorInvalidValue;
    const double4* tri = (const double4*)tri12;
    const dim3 per_query((unsigned)((nq + 255) / 256)), nt(256);
    hipLaunchKernelGGL(k_tri_fill, per_query, nt, 0, s, sq, key, (long long)nq, counters);
    hipLaunchKernelGGL((k_tri_min<kTriQpt, false, false>), dim3((unsigned)n_a), nt, 0, s, work, n_a, tri, nf, qxyz, nq, sq,
                       key, counters);
    if (n_b > 0)
        hipLaunchKernelGGL((k_tri_min<kTriQpt, true, false>), dim3((unsigned)n_b), nt, 0, s, work + n_a, n_b, tri, nf, qxyz,
                           nq, sq, key, counters);
    hipLaunchKernelGGL((k_tri_min<kTriQpt, false, true>), dim3((unsigned)(n_a + n_b)), nt, 0, s, work, n_a + n_b, tri, nf,
                       qxyz, nq, sq, key, counters);
    hipLaunchKernelGGL(k_tri_closest, per_query, nt, 0, s, tri, qxyz, nq, key, closest, region);
    return hipGetLastError();
}

int tri_launches(int n_b) { return n_b > 0 ? 5 : 4; }

// The same search over seeded minima: sq holds, per query, the bits of the d2 to one face of the set (face_d2 of
// mm_tri_device.h: a member of the fold), key ~0.  The minimum of the set is then the minimum of the seed and the items,
// so every one of the n_work items runs checked (counters[0] += those skipped), the who pass and the closest points
// follow: tri_seeded_launches() kernels.
hipError_t launch_tri_seeded(const TriWork* work, int n_work, const double* tri12, int nf, const double* qxyz, int nq,
                             unsigned long long* sq, unsigned long long* key, double* closest, int32_t* region,
                             unsigned long long* counters, hipStream_t s)
{
    if (nq <= 0 || nf <= 0 || n_work <= 0) return hipErrorInvalidValue;
    const double4* tri = (const double4*)tri12;
    const dim3 per_query((unsigned)((nq + 255) / 256)), nt(256);
    hipLaunchKernelGGL((k_tri_min<kTriQpt, true, false>), dim3((unsigned)n_work), nt, 0, s, work, n_work, tri, nf, qxyz, nq,
                       sq, key, counters);
    hipLaunchKernelGGL((k_tri_min<kTriQpt, false, true>), dim3((unsigned)n_work), nt, 0, s, work, n_work, tri, nf, qxyz, nq,
                       sq, key, counters);
    hipLaunchKernelGGL(k_tri_closest, per_query, nt, 0, s, tri, qxyz, nq, key, closest, region);
    return hipGetLastError();
}

int tri_seeded_launches() { return 3; }

}  // namespace mm
