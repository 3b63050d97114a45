// mm_winding_kernels.hip -- the generalized winding number of a triangle mesh at query points, f64, for gfx950: the rule
// of include/mm_ccta.h ("winding number"), whose arithmetic is mm_winding_device.h.  No atan2 on the device: a running
// angle is an integer number of quarter turns and a complex number kept in the cone re >= |im|, so the result is a
// function of +, -, *, /, sqrt, comparisons and exact power-of-two scalings and has the checker's bits.
//
// Mapping (as k_tri_min of mm_tri_kernels.hip): one work item = 256 lanes x kQpt queries against one group of G
// consecutive chunks of 256 staged faces.  A chunk is staged in LDS as 9 doubles a face; every lane reads the same
// corner (a broadcast: conflict-free).  A lane keeps, per query, p, n, pr, pi, rho and touch in registers and folds the
// group's faces in staged order from (0, (1, 0)); it writes one 32-byte partial record per (query, group) at
// part[group * nq + query].  No atomics, no float reduction: the fold order is fixed by the rule, not by the schedule.
// k_wind_join then folds each query's group partials in ascending order, one lane per query.
// Per (query, face): about 90 fp64 operations, three square roots and one division against 9 / kQpt LDS reads ->
// fp64-VALU bound.
#include <hip/hip_runtime.h>

#include "mm_device.h"
#include "mm_winding_device.h"

namespace mm {

using winding::State;

static constexpr int kWindChunk = winding::kChunk;
static constexpr int kWindQpt = winding::kQpt;

// tri9: nf staged faces, 9 doubles each; the block's group is blockIdx.x % groups, its query block blockIdx.x / groups
__global__ void __launch_bounds__(256)
k_wind_partial(const double* __restrict__ tri9, int nf, int chunks_per_group, int groups, const double* __restrict__ qxyz,
               int nq, State* __restrict__ part)
{
    constexpr int NT = 256, CH = kWindChunk, QPT = kWindQpt;
    __shared__ double s_t[9 * CH];
    const int tid = threadIdx.x;
    const int g = (int)(blockIdx.x % (unsigned)groups);
    const int q0 = (int)(blockIdx.x / (unsigned)groups) * (NT * QPT);
    double px[QPT], py[QPT], pz[QPT];
    State st[QPT];
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
        const int q = q0 + k * NT + tid;
        const int qc = q < nq ? q : nq - 1;   // lanes past the end recompute the last query, never stored
        px[k] = qxyz[3 * (long long)qc]; py[k] = qxyz[3 * (long long)qc + 1]; pz[k] = qxyz[3 * (long long)qc + 2];
        st[k] = winding::start();
    }
    const long long f0 = (long long)g * chunks_per_group * CH;
    long long f1 = f0 + (long long)chunks_per_group * CH;
    f1 = f1 < nf ? f1 : nf;
    for (long long c0 = f0; c0 < f1; c0 += CH) {
        const int n = (int)(f1 - c0 < CH ? f1 - c0 : CH);
        __syncthreads();   // previous chunk fully consumed
        for (int j = tid; j < 9 * n; j += NT) s_t[j] = tri9[9 * c0 + j];
        __syncthreads();
        for (int j = 0; j < n; ++j) {
            const double* t = s_t + 9 * j;
            const double ax = t[0], ay = t[1], az = t[2], bx = t[3], by = t[4], bz = t[5], cx = t[6], cy = t[7], cz = t[8];
#pragma unroll
            for (int k = 0; k < QPT; ++k) winding::face(st[k], px[k], py[k], pz[k], ax, ay, az, bx, by, bz, cx, cy, cz);
        }
    }
#pragma unroll
    for (int k = 0; k < QPT; ++k) {
        const int q = q0 + k * NT + tid;
        if (q < nq) part[(long long)g * nq + q] = st[k];
    }
}

// one lane per query: its group partials in ascending order
__global__ void __launch_bounds__(256)
k_wind_join(const State* __restrict__ part, int groups, int nq, int32_t* __restrict__ out_n, double* __restrict__ out_p,
            double* __restrict__ out_rho, int32_t* __restrict__ out_touch)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= nq) return;
    State s = part[q];
    for (int g = 1; g < groups; ++g) winding::join(s, part[(long long)g * nq + q]);
    out_n[q] = s.n;
    out_p[2 * (long long)q] = s.pr; out_p[2 * (long long)q + 1] = s.pi;
    out_rho[q] = s.rho;
    out_touch[q] = s.touch;
}

int wind_queries_per_block() { return 256 * kWindQpt; }
int wind_chunk_faces() { return kWindChunk; }
int wind_max_groups() { return winding::kMaxGroups; }
int wind_launches() { return 2; }

hipError_t launch_winding(const double* tri9, int nf, int chunks_per_group, int groups, const double* qxyz, int nq,
                          void* partials, int32_t* out_n, double* out_p, double* out_rho, int32_t* out_touch, hipStream_t s)
{
    if (nq <= 0 || nf <= 0 || chunks_per_group <= 0 || groups <= 0 || groups > winding::kMaxGroups) return hipErrorInvalidValue;
    if ((long long)(groups - 1) * chunks_per_group * kWindChunk >= nf) return hipErrorInvalidValue;   // no empty group
    const long long qblocks = ((long long)nq + 256 * kWindQpt - 1) / (256 * kWindQpt);
    if (qblocks * groups > 0x7fffffffll) return hipErrorInvalidValue;
    State* part = (State*)partials;
    hipLaunchKernelGGL(k_wind_partial, dim3((unsigned)(qblocks * groups)), dim3(256), 0, s, tri9, nf, chunks_per_group, groups,
                       qxyz, nq, part);
    hipLaunchKernelGGL(k_wind_join, dim3((unsigned)((nq + 255) / 256)), dim3(256), 0, s, part, groups, nq, out_n, out_p, out_rho,
                       out_touch);
    return hipGetLastError();
}

}  // namespace mm
