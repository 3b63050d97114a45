// mm_ray_kernels.hip -- ray casting of the occlusion removal of CCTA mesh labelling, exact f64, for gfx950.
//
// remove_occluded_points_ray_triangle (src/ccta/adjust_mesh/label_coronary.rs:70-197) casts a ray from every aortic
// centerline point to every step-th coronary centerline point near the ostium and tests it against every candidate
// face with Moeller-Trumbore (ray_triangle_intersection, :29-68).  Per ray it needs the number of faces hit and the
// face of the smallest t (the first after a stable sort by t: ties go to the lowest face index).
//
// The test is restated in the reference's operation order: cross(a, b) = (ay bz - az by, az bx - ax bz, ax by - ay bx),
// dot(a, b) = (ax bx + ay by) + az bz, f = 1 / a a correctly rounded division (v_div_scale / v_div_fmas /
// v_div_fixup, no reciprocal shortcut), no contraction (the file is built with -ffp-contract=off) and every NaN
// comparison false, as in Rust.  edge1 = v1 - v0 and edge2 = v2 - v0 are the same roundings per face whichever ray
// asks, so the host stages them once.
//
// Mapping: one work item = 256 rays (one per lane) x one chunk of kRayChunk faces, staged in LDS as 9 planes
// (v0, e1, e2) that every lane reads at the same address (broadcast, conflict-free).  Each lane keeps its hit count
// and the lexicographic minimum of (t, face index) over the chunk and writes them to a per-(chunk, ray) partial slab;
// k_ray_fold then walks each ray's partials in chunk order.  No atomics: the result is deterministic and does not
// depend on the schedule.  Work items are chunk-major (the blocks of one chunk share its faces in L2) and dealt to
// the XCDs in contiguous eighths.
#include <hip/hip_runtime.h>

#include "mm_device.h"
#include "mm_xcd.h"

namespace mm {

static constexpr int kRayChunk = 256;   // faces per LDS chunk (9 x 256 doubles = 18 KiB)
static constexpr int kRayLanes = 256;   // rays per work item

// ray: 6 planes of n_rays doubles (origin xyz, direction xyz); tri: 9 planes of n_faces doubles (v0 xyz, e1 xyz, e2 xyz)
__global__ void __launch_bounds__(256)
k_ray_tri(const double* __restrict__ ray, int n_rays, const double* __restrict__ tri, int n_faces, int n_rblk,
          int n_work, RayPartial* __restrict__ part)
{
    __shared__ double s_f[9][kRayChunk];
    const int tid = threadIdx.x;
    const size_t nr = (size_t)n_rays, nf = (size_t)n_faces;
    for (int wi = (int)gridDim.x == n_work ? xcd_work_index(blockIdx.x, n_work) : (int)blockIdx.x; wi < n_work;
         wi += gridDim.x) {
        const int chunk = wi / n_rblk, rb = wi - chunk * n_rblk;
        const int f0 = chunk * kRayChunk;
        const int n = n_faces - f0 < kRayChunk ? n_faces - f0 : kRayChunk;
        __syncthreads();   // the previous item's chunk is fully consumed
        for (int j = tid; j < n; j += kRayLanes)
#pragma unroll
            for (int k = 0; k < 9; ++k) s_f[k][j] = tri[(size_t)k * nf + (size_t)(f0 + j)];
        __syncthreads();
        const int r = rb * kRayLanes + tid;
        const size_t rc = (size_t)(r < n_rays ? r : n_rays - 1);   // lanes past the end recompute the last ray, never stored
        const double ox = ray[rc], oy = ray[nr + rc], oz = ray[2 * nr + rc];
        const double dx = ray[3 * nr + rc], dy = ray[4 * nr + rc], dz = ray[5 * nr + rc];
        int cnt = 0, best_f = -1;
        double best_t = __builtin_inf();
        for (int j = 0; j < n; ++j) {
            const double v0x = s_f[0][j], v0y = s_f[1][j], v0z = s_f[2][j];
            const double e1x = s_f[3][j], e1y = s_f[4][j], e1z = s_f[5][j];
            const double e2x = s_f[6][j], e2y = s_f[7][j], e2z = s_f[8][j];
            // h = d x edge2, a = edge1 . h (:41-42)
            const double hx = dy * e2z - dz * e2y, hy = dz * e2x - dx * e2z, hz = dx * e2y - dy * e2x;
            const double a = (e1x * hx + e1y * hy) + e1z * hz;
            if (__builtin_fabs(a) < 1e-8) continue;                          // :43-45 parallel
            const double f = 1.0 / a;                                         // :47
            const double sx = ox - v0x, sy = oy - v0y, sz = oz - v0z;         // :48
            const double u = f * ((sx * hx + sy * hy) + sz * hz);             // :50
            if (!(u >= 0.0 && u <= 1.0)) continue;                            // :51-53 (NaN rejects)
            const double qx = sy * e1z - sz * e1y, qy = sz * e1x - sx * e1z, qz = sx * e1y - sy * e1x;   // :55
            const double v = f * ((dx * qx + dy * qy) + dz * qz);             // :57
            if (v < 0.0 || u + v > 1.0) continue;                             // :58-60 (NaN passes, as in Rust)
            const double t = f * ((e2x * qx + e2y * qy) + e2z * qz);          // :63
            if (t > 1e-8) {                                                   // :64
                ++cnt;
                if (t < best_t) { best_t = t; best_f = f0 + j; }              // faces ascend: ties keep the lowest index
            }
        }
        if (r < n_rays) part[(size_t)chunk * nr + (size_t)r] = RayPartial{cnt, best_f, best_t};
    }
}

// closest[r] = the face of the smallest (t, index) of ray r if it hits at least 3 faces (:131-135), else -1
__global__ void __launch_bounds__(256)
k_ray_fold(const RayPartial* __restrict__ part, int n_rays, int n_chunks, int32_t* __restrict__ closest)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n_rays) return;
    long long cnt = 0;
    int best_f = -1;
    double best_t = __builtin_inf();
    for (int c = 0; c < n_chunks; ++c) {
        const RayPartial p = part[(size_t)c * (size_t)n_rays + (size_t)r];
        cnt += p.count;
        if (p.count > 0 && p.t < best_t) { best_t = p.t; best_f = p.face; }   // earlier chunks hold lower indices
    }
    closest[r] = cnt >= 3 ? best_f : -1;
}

int ray_chunk_faces() { return kRayChunk; }
int ray_block_rays() { return kRayLanes; }

hipError_t launch_ray_tri(const double* ray, int n_rays, const double* tri, int n_faces, RayPartial* part,
                          int32_t* closest, hipStream_t s)
{
    if (n_rays <= 0) return hipSuccess;
    const int n_rblk = (n_rays + kRayLanes - 1) / kRayLanes;
    const int n_chunks = n_faces > 0 ? (n_faces + kRayChunk - 1) / kRayChunk : 0;
    const long long n_work = (long long)n_rblk * n_chunks;
    if (n_work > 0x7fffffffLL) return hipErrorInvalidValue;
    if (n_work > 0)
        hipLaunchKernelGGL(k_ray_tri, dim3((unsigned)n_work), dim3(256), 0, s, ray, n_rays, tri, n_faces, n_rblk,
                           (int)n_work, part);
    hipLaunchKernelGGL(k_ray_fold, dim3((unsigned)n_rblk), dim3(256), 0, s, part, n_rays, n_chunks, closest);
    return hipGetLastError();
}

}  // namespace mm
