// mm_section_kernels.hip -- exact plane cuts of a triangle mesh, f64, for gfx950: the device step of "mesh
// cross-sections" (include/mm_ccta.h).  Every (plane, face) pair that the host's cull leaves is tested; every crossed
// face gives one segment record whose bits are a pure function of the plane and the face (mm_section_device.h; the
// file is built with -ffp-contract=off), so the chunking, the plane runs and the order of arrival cannot change a bit.
//
// Mapping: one work item = a chunk of 256 faces in slab order against a run of at most 64 of the planes that pass the
// chunk's box (rule 8).  One workgroup of 256 lanes per item.  A lane keeps one face in registers: nine doubles, three
// vertex indices and the original face index.  The run's planes sit in LDS, 64 x 48 bytes; all lanes read the same
// address (a broadcast, conflict-free).  Per (lane, plane): three heights and the side test.  The few crossed lanes
// compute their two points under divergence and append a record through a wave-aggregated reservation: a ballot, one
// atomicAdd of the popcount by the first crossed lane, the rank inside the wave by mbcnt.  Records beyond `cap` are
// dropped; the count is always complete.  k_section_clear zeroes the counters on every call; the host reads no record
// above the count.
#include <hip/hip_runtime.h>

#include "mm_device.h"
#include "mm_section_device.h"

namespace mm {

static constexpr int kSectionChunk = section::kChunk;
static constexpr int kSectionPlaneRun = 64;   // 64 planes x 48 bytes = 3 KiB of LDS
static_assert(kSectionPlaneRun == section::kPlaneRun, "the host cuts the plane lists into runs of this length");

__device__ __forceinline__ unsigned long long section_first_lane(unsigned long long v)
{
    const unsigned int lo = __builtin_amdgcn_readfirstlane((unsigned int)v);
    const unsigned int hi = __builtin_amdgcn_readfirstlane((unsigned int)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

__global__ void __launch_bounds__(64)
k_section_clear(unsigned long long* __restrict__ counters)
{
    if (threadIdx.x < 8) counters[threadIdx.x] = 0ull;
}

__global__ void __launch_bounds__(256)
k_section_cut(const int4* __restrict__ items, int n_items, const int* __restrict__ plane_list,
              const double* __restrict__ planes, const double4* __restrict__ tri, int n_faces,
              unsigned long long* __restrict__ counters, section::Segment* __restrict__ out, unsigned long long cap)
{
    using namespace section;
    __shared__ double s_pl[6 * kSectionPlaneRun];
    const int tid = threadIdx.x;
    for (int wi = blockIdx.x; wi < n_items; wi += gridDim.x) {
        const int4 it = items[wi];                                     // chunk, first entry of the plane list, planes
        const int i = it.x * kSectionChunk + tid;
        const int ic = i < n_faces ? i : n_faces - 1;                  // lanes past the end hold the last face, not live
        const double4 la = tri[3 * (long long)ic], lb = tri[3 * (long long)ic + 1], lc = tri[3 * (long long)ic + 2];
        const unsigned long long wa = (unsigned long long)__double_as_longlong(la.w);
        const unsigned long long wb = (unsigned long long)__double_as_longlong(lb.w);
        const int id0 = (int)(unsigned int)wa, id1 = (int)(wa >> 32), id2 = (int)(unsigned int)wb;
        const unsigned long long orig = wb >> 32;
        const bool live = i < n_faces && __double_as_longlong(lc.w) == 0;   // a face with a repeated index is skipped
        const int np = it.z < kSectionPlaneRun ? it.z : kSectionPlaneRun;
        __syncthreads();                                               // the previous run fully consumed
        for (int j = tid; j < 6 * np; j += 256) s_pl[j] = planes[6 * (long long)plane_list[it.y + j / 6] + j % 6];
        __syncthreads();
        for (int k = 0; k < np; ++k) {
            const Plane pl{s_pl[6 * k], s_pl[6 * k + 1], s_pl[6 * k + 2], s_pl[6 * k + 3], s_pl[6 * k + 4], s_pl[6 * k + 5]};
            const double h0 = height(pl, la.x, la.y, la.z), h1 = height(pl, lb.x, lb.y, lb.z), h2 = height(pl, lc.x, lc.y, lc.z);
            const bool hit = live && crossed(h0, h1, h2);
            const unsigned long long mask = __ballot(hit);
            if (mask == 0ull) continue;                                // uniform: most planes miss most waves
            if (hit) {
                const unsigned int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(mask >> 32),
                                                                    __builtin_amdgcn_mbcnt_lo((unsigned int)mask, 0u));
                unsigned long long base = 0ull;
                if (rank == 0u) base = atomicAdd(&counters[0], (unsigned long long)__popcll(mask));
                base = section_first_lane(base);                       // the first crossed lane is the one of rank 0
                const unsigned long long slot = base + rank;
                if (slot < cap) {
                    const unsigned long long plane = (unsigned long long)(unsigned int)plane_list[it.y + k];
                    Segment s;
                    cut_face(Corner{la.x, la.y, la.z, h0, id0}, Corner{lb.x, lb.y, lb.z, h1, id1},
                             Corner{lc.x, lc.y, lc.z, h2, id2}, (plane << 32) | orig, s);
                    out[slot] = s;
                }
            }
        }
    }
}

int section_launches() { return 2; }

hipError_t launch_section_cut(const int32_t* items, int n_items, const int32_t* plane_list, const double* planes,
                              const double* tri12, int n_faces, unsigned long long* counters, void* segments,
                              unsigned long long cap, hipStream_t s)
{
    if (n_items <= 0 || n_faces <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_section_clear, dim3(1), dim3(64), 0, s, counters);
    const dim3 grid((unsigned)(n_items < (1 << 20) ? n_items : (1 << 20)));
    hipLaunchKernelGGL(k_section_cut, grid, dim3(256), 0, s, (const int4*)items, n_items, plane_list, planes,
                       (const double4*)tri12, n_faces, counters, (section::Segment*)segments, cap);
    return hipGetLastError();
}

}  // namespace mm
