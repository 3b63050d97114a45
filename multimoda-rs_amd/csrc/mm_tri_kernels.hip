// mm_tri_kernels.hip -- exact point-to-triangle squared distances in 3-D, f64, for gfx950: the surface distance of
// include/mm_ccta.h ("surface distance").  For every query p:  out[p] = min_f d2(p, face f), with d2 the squared distance
// to Ericson's closest point (Real-Time Collision Detection 5.1.5), every operation unfused and in the header's order
// (the file is built with -ffp-contract=off), every quotient a true division.  min is exact, so the result does not
// depend on the traversal order.
//
// Mapping: one work item = 256 lanes x QPT queries against one chunk of CH faces; a chunk is staged in LDS as three
// double4 per face (corner a, b, c), so that a corner is two ds_read broadcasts (all lanes read the same address:
// conflict-free).  a.w carries the bits of the face's degenerate flag, b.w those of its original index; both are the
// same for all lanes and are made scalar with readfirstlane, so the degenerate branch is uniform.
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
#include "mm_xcd.h"

namespace mm {

static constexpr int kTriChunk = 256;   // 256 faces x 3 double4 = 24 KiB of LDS: 6 blocks a CU by LDS
static constexpr int kTriQpt = 2;

struct V3 { double x, y, z; };

__device__ __forceinline__ V3 sub3(const V3& u, const V3& v) { return V3{u.x - v.x, u.y - v.y, u.z - v.z}; }
__device__ __forceinline__ double dot3(const V3& u, const V3& v) { return (u.x * v.x + u.y * v.y) + u.z * v.z; }
// u + e * t, one rounding for each product and each sum
__device__ __forceinline__ V3 along(const V3& u, const V3& e, double t) { return V3{u.x + e.x * t, u.y + e.y * t, u.z + e.z * t}; }
__device__ __forceinline__ double dist2(const V3& p, const V3& q) { const V3 d = sub3(p, q); return dot3(d, d); }

// closest point of a proper face; ab = b - a, ac = c - a
__device__ __forceinline__ V3 tri_closest(const V3& p, const V3& a, const V3& b, const V3& c, const V3& ab, const V3& ac,
                                          int& region)
{
    const V3 ap = sub3(p, a);
    const double d1 = dot3(ab, ap), d2 = dot3(ac, ap);
    if (d1 <= 0.0 && d2 <= 0.0) { region = 1; return a; }
    const V3 bp = sub3(p, b);
    const double d3 = dot3(ab, bp), d4 = dot3(ac, bp);
    if (d3 >= 0.0 && d4 <= d3) { region = 2; return b; }
    const double vc = d1 * d4 - d3 * d2;
    if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) { region = 4; return along(a, ab, d1 / (d1 - d3)); }
    const V3 cp = sub3(p, c);
    const double d5 = dot3(ab, cp), d6 = dot3(ac, cp);
    if (d6 >= 0.0 && d5 <= d6) { region = 3; return c; }
    const double vb = d5 * d2 - d1 * d6;
    if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) { region = 6; return along(a, ac, d2 / (d2 - d6)); }
    const double va = d3 * d6 - d5 * d4;
    const double e43 = d4 - d3, e56 = d5 - d6;
    if (va <= 0.0 && e43 >= 0.0 && e56 >= 0.0) { region = 5; return along(b, sub3(c, b), e43 / (e43 + e56)); }
    const double s = (va + vb) + vc;
    region = 0;
    return along(along(a, ab, vb / s), ac, vc / s);
}

// closest point of the segment (u, v)
__device__ __forceinline__ V3 seg_closest(const V3& p, const V3& u, const V3& v)
{
    const V3 e = sub3(v, u);
    const double l = dot3(e, e);
    double t = 0.0;
    if (l != 0.0) {
        t = dot3(sub3(p, u), e) / l;
        t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);   // a NaN stays a NaN
    }
    return along(u, e, t);
}

// closest point of a degenerate face: the nearest of ab, bc, ca, the first on ties
__device__ __forceinline__ V3 degenerate_closest(const V3& p, const V3& a, const V3& b, const V3& c, int& region)
{
    V3 q = seg_closest(p, a, b);
    double best = dist2(p, q);
    region = 4;
    const V3 q2 = seg_closest(p, b, c);
    const double v2 = dist2(p, q2);
    if (v2 < best) { best = v2; q = q2; region = 5; }
    const V3 q3 = seg_closest(p, c, a);
    const double v3 = dist2(p, q3);
    if (v3 < best) { q = q3; region = 6; }
    return q;
}

__device__ __forceinline__ double face_d2(const V3& p, const V3& a, const V3& b, const V3& c, const V3& ab, const V3& ac,
                                          bool degenerate)
{
    int region;
    const V3 q = degenerate ? degenerate_closest(p, a, b, c, region) : tri_closest(p, a, b, c, ab, ac, region);
    return dist2(p, q);
}

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
            const bool degenerate = scalar_bits(ta.w) != 0ull;
            const unsigned long long id = WHO ? (scalar_bits(tb.w) << 32) | (unsigned int)(w.c0 + j) : 0ull;
#pragma unroll
            for (int k = 0; k < QPT; ++k) {
                const double v = face_d2(p[k], a, b, c, ab, ac, degenerate);
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
        c = __double_as_longlong(ta.w) != 0 ? degenerate_closest(p, a, b, cc, r)
                                            : tri_closest(p, a, b, cc, sub3(b, a), sub3(cc, a), r);
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

}  // namespace mm
