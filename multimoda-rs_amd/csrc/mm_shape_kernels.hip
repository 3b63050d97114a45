// mm_shape_kernels.hip -- lumen morphometry of a batch of contours, exact f64, for gfx950.
//
// Per contour of n points p_0 .. p_{n-1} (src/types/native/contour.rs, distances src/types/native.rs:27-39):
//   farthest pair (:227-242)   max over i < j of s_ij = sqrt((dx^2 + dy^2) + dz^2), from (0.0, pair (0, 0)), replaced
//                              on a strictly larger s in (i asc, j asc) order: the lexicographically first pair of the
//                              largest s; NaN never wins.  Lanes screen on the squared distance (see below).
//   closest opposite 3-D       min over i of s_{i, (i + n/2) % n}, from (DBL_MAX, pair (0, n/2)), replaced on a
//   (:313-333)                 strictly smaller value: the first minimum.
//   closest opposite 2-D       theta_i (host: std::atan2 about the centre, + 2 pi below 0) arrives in `theta`.  For
//   (:247-310)                 each i, j != i in order: delta = |theta_j - theta_i|, 2 pi - delta above pi, diff =
//                              |delta - pi|, best_j on a strictly smaller diff from DBL_MAX (best_j = i if none);
//                              then sqrt(dx^2 + dy^2) of (i, best_j), min over i from (DBL_MAX, pair (0, 1)).
//   area (:345-361)            three sequential cross-product sums over (p_i, p_{(i+1) % n}), 0.5 * sqrt((cx^2 + cy^2)
//                              + cz^2); 0.0 for n < 3.  One lane, index order.
//   elliptic ratio (:335-343)  major < minor_3d ? minor_3d / major : major / minor_3d.
// No contraction (the file is built with -ffp-contract=off); sqrt and the division are hipcc's correctly rounded
// expansions, so every value is the reference's bit for bit.
//
// Squared-distance screen of the farthest pair: sqrt is monotonic, so a pair can only raise a lane's best s if its d2
// exceeds the largest d2 the lane has seen so far (`scr`); only then is the sqrt taken, and the pair replaces the best
// only if its s is strictly larger.  So s_best == sqrt(scr) throughout, and the lane keeps the FIRST pair (in its own
// visiting order) of its largest s -- a later pair whose distinct d2 rounds to the same s does not win, as in the
// reference.  Each lane visits segments in lexicographic order (row r, then row n - 1 - r: the triangle balanced to
// n - 1 pairs per lane); segments merge, and lanes reduce, by (s desc, i asc, j asc).
//
// Mapping: one workgroup of 256 lanes per contour, contours dealt to the XCDs in contiguous eighths.  Contours of up
// to kShapeLds points are staged in LDS as x / y / z / theta arrays (32 KiB; 43 KiB with the reduction, three
// workgroups per CU); larger ones are read from global memory (same arithmetic, same order).  The three folds reduce
// through LDS; no atomics.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <climits>

#include "mm_device.h"
#include "mm_xcd.h"

namespace mm {

static constexpr int kShapeLanes = 256;
static constexpr int kShapeLds = 1024;   // points staged in LDS: 4 arrays x 1024 x 8 B = 32 KiB
static constexpr double kPi = 3.14159265358979323846;

struct LdsPts {
    const double *x, *y, *z, *t;
    __device__ __forceinline__ double X(int j) const { return x[j]; }
    __device__ __forceinline__ double Y(int j) const { return y[j]; }
    __device__ __forceinline__ double Z(int j) const { return z[j]; }
    __device__ __forceinline__ double T(int j) const { return t[j]; }
};
struct GlobalPts {
    const double* __restrict__ p;   // xyz rows of this contour
    const double* __restrict__ t;
    __device__ __forceinline__ double X(int j) const { return p[3 * (size_t)j]; }
    __device__ __forceinline__ double Y(int j) const { return p[3 * (size_t)j + 1]; }
    __device__ __forceinline__ double Z(int j) const { return p[3 * (size_t)j + 2]; }
    __device__ __forceinline__ double T(int j) const { return t[j]; }
};

// (s desc, i asc, j asc)
static __device__ __forceinline__ bool far_better(double s, int i, int j, double bs, int bi, int bj)
{
    return s > bs || (s == bs && (i < bi || (i == bi && j < bj)));
}
// (d asc, i asc); an empty slot is (DBL_MAX, INT_MAX)
static __device__ __forceinline__ bool near_better(double d, int i, double bd, int bi)
{
    return d < bd || (d == bd && i < bi);
}

struct ShapeRed {
    double fs[kShapeLanes], m3[kShapeLanes], m2[kShapeLanes];
    int fi[kShapeLanes], fj[kShapeLanes], m3i[kShapeLanes], m2i[kShapeLanes], m2j[kShapeLanes];
};

// row i against j in [j0, j1) of one segment: the squared-distance screen (see the header)
template <class P>
static __device__ __forceinline__ void far_row(const P& P_, int i, int j0, int j1, double& scr, double& bs, int& bi,
                                               int& bj)
{
    const double px = P_.X(i), py = P_.Y(i), pz = P_.Z(i);
#pragma unroll 4
    for (int j = j0; j < j1; ++j) {
        const double dx = px - P_.X(j), dy = py - P_.Y(j), dz = pz - P_.Z(j);
        const double d2 = dx * dx + dy * dy + dz * dz;
        if (d2 > scr) {
            scr = d2;
            const double s = sqrt(d2);
            if (s > bs) { bs = s; bi = i; bj = j; }
        }
    }
}

template <class P>
static __device__ __forceinline__ void shape_body(const P& P_, int n, bool want2d, ShapeRed& R, double* __restrict__ val,
                                                  long long* __restrict__ idx)
{
    const int tid = threadIdx.x;
    // ---- farthest pair: lane takes row pairs r = tid, tid + 256, ...; row r and row n - 1 - r form one segment
    double fs = 0.0;
    int fi = 0, fj = 0;
    for (int r = tid; r < (n + 1) / 2; r += kShapeLanes) {
        const int hi = n - 1 - r;
        double scr = 0.0, bs = 0.0;
        int bi = 0, bj = 0;
        far_row(P_, r, r + 1, n, scr, bs, bi, bj);
        if (hi != r) far_row(P_, hi, hi + 1, n, scr, bs, bi, bj);
        if (far_better(bs, bi, bj, fs, fi, fj)) { fs = bs; fi = bi; fj = bj; }
    }
    // ---- closest opposite, 3-D
    const int half = n / 2;
    double m3 = DBL_MAX;
    int m3i = INT_MAX;
    if (n >= 3) {
        for (int i = tid; i < n; i += kShapeLanes) {
            int j = i + half;
            if (j >= n) j -= n;
            const double dx = P_.X(i) - P_.X(j), dy = P_.Y(i) - P_.Y(j), dz = P_.Z(i) - P_.Z(j);
            const double d = sqrt(dx * dx + dy * dy + dz * dz);
            if (d < m3) { m3 = d; m3i = i; }
        }
    }
    // ---- closest opposite, 2-D
    double m2 = DBL_MAX;
    int m2i = INT_MAX, m2j = INT_MAX;
    if (want2d && n >= 3) {
        for (int i = tid; i < n; i += kShapeLanes) {
            const double ti = P_.T(i);
            double bd = DBL_MAX;
            int bj = i;
            for (int j = 0; j < n; ++j) {
                double delta = fabs(P_.T(j) - ti);
                if (delta > kPi) delta = 2.0 * kPi - delta;
                const double diff = fabs(delta - kPi);
                if (diff < bd && j != i) { bd = diff; bj = j; }
            }
            const double dx = P_.X(i) - P_.X(bj), dy = P_.Y(i) - P_.Y(bj);
            const double d = sqrt(dx * dx + dy * dy);
            if (d < m2) { m2 = d; m2i = i; m2j = bj; }
        }
    }
    // ---- area: one lane, index order (the last lane: the farthest pair leaves it idle up to n = 510)
    double area = 0.0;
    if (tid == kShapeLanes - 1 && n >= 3) {
        double cx = 0.0, cy = 0.0, cz = 0.0;
        for (int i = 0; i < n; ++i) {
            const int k = i + 1 == n ? 0 : i + 1;
            const double x1 = P_.X(i), y1 = P_.Y(i), z1 = P_.Z(i), x2 = P_.X(k), y2 = P_.Y(k), z2 = P_.Z(k);
            cx += y1 * z2 - z1 * y2;
            cy += z1 * x2 - x1 * z2;
            cz += x1 * y2 - y1 * x2;
        }
        area = 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
    }
    // ---- reduce the three folds across the workgroup
    R.fs[tid] = fs; R.fi[tid] = fi; R.fj[tid] = fj;
    R.m3[tid] = m3; R.m3i[tid] = m3i;
    R.m2[tid] = m2; R.m2i[tid] = m2i; R.m2j[tid] = m2j;
    __syncthreads();
    for (int st = kShapeLanes / 2; st > 0; st >>= 1) {
        if (tid < st) {
            const int o = tid + st;
            if (far_better(R.fs[o], R.fi[o], R.fj[o], R.fs[tid], R.fi[tid], R.fj[tid])) {
                R.fs[tid] = R.fs[o]; R.fi[tid] = R.fi[o]; R.fj[tid] = R.fj[o];
            }
            if (near_better(R.m3[o], R.m3i[o], R.m3[tid], R.m3i[tid])) { R.m3[tid] = R.m3[o]; R.m3i[tid] = R.m3i[o]; }
            if (near_better(R.m2[o], R.m2i[o], R.m2[tid], R.m2i[tid])) {
                R.m2[tid] = R.m2[o]; R.m2i[tid] = R.m2i[o]; R.m2j[tid] = R.m2j[o];
            }
        }
        __syncthreads();
    }
    if (tid == kShapeLanes - 1) val[0] = area;
    if (tid == 0) {
        const double nan = __builtin_nan("");
        if (n == 0) { val[1] = nan; idx[0] = -1; idx[1] = -1; }
        else { val[1] = R.fs[0]; idx[0] = R.fi[0]; idx[1] = R.fj[0]; }
        if (n < 3) {
            val[2] = nan; val[3] = nan; val[4] = nan;
            idx[2] = idx[3] = idx[4] = idx[5] = -1;
        } else {
            const double major = R.fs[0];
            double minor = DBL_MAX;
            if (R.m3i[0] == INT_MAX) { idx[2] = 0; idx[3] = half; }   // no distance below DBL_MAX: the initial pair
            else {
                minor = R.m3[0];
                idx[2] = R.m3i[0];
                idx[3] = R.m3i[0] + half >= n ? R.m3i[0] + half - n : R.m3i[0] + half;
            }
            val[2] = minor;
            val[4] = major < minor ? minor / major : major / minor;
            if (!want2d) { val[3] = nan; idx[4] = idx[5] = -1; }
            else if (R.m2i[0] == INT_MAX) { val[3] = DBL_MAX; idx[4] = 0; idx[5] = 1; }
            else { val[3] = R.m2[0]; idx[4] = R.m2i[0]; idx[5] = R.m2j[0]; }
        }
    }
}

// xyz: point rows of all contours; theta: one angle per point (read only when want2d); val: 5 per contour (area,
// major, minor 3-D, minor 2-D, elliptic ratio); idx: 6 per contour (the three pairs, contour-local)
__global__ void __launch_bounds__(256)
k_contour_measures(const ShapeJob* __restrict__ jobs, int n_jobs, const double* __restrict__ xyz,
                   const double* __restrict__ theta, int want2d, double* __restrict__ val, long long* __restrict__ idx)
{
    __shared__ double s_x[kShapeLds], s_y[kShapeLds], s_z[kShapeLds], s_t[kShapeLds];
    __shared__ ShapeRed s_red;
    const int tid = threadIdx.x;
    for (int wi = (int)gridDim.x == n_jobs ? xcd_work_index(blockIdx.x, n_jobs) : (int)blockIdx.x; wi < n_jobs;
         wi += gridDim.x) {
        const ShapeJob jb = jobs[wi];
        const double* p = xyz + 3 * (size_t)jb.off;
        const double* t = want2d ? theta + (size_t)jb.off : nullptr;
        __syncthreads();   // the previous contour is fully consumed
        if (jb.n <= kShapeLds) {
            for (int j = tid; j < jb.n; j += kShapeLanes) {
                s_x[j] = p[3 * (size_t)j];
                s_y[j] = p[3 * (size_t)j + 1];
                s_z[j] = p[3 * (size_t)j + 2];
                s_t[j] = want2d ? t[j] : 0.0;
            }
            __syncthreads();
            shape_body(LdsPts{s_x, s_y, s_z, s_t}, jb.n, want2d != 0, s_red, val + 5 * (size_t)wi, idx + 6 * (size_t)wi);
        } else {
            shape_body(GlobalPts{p, t}, jb.n, want2d != 0, s_red, val + 5 * (size_t)wi, idx + 6 * (size_t)wi);
        }
    }
}

hipError_t launch_contour_measures(const ShapeJob* jobs, int n_jobs, const double* xyz, const double* theta, int want2d,
                                   double* val, int64_t* idx, hipStream_t s)
{
    if (n_jobs <= 0) return hipSuccess;
    const int grid = n_jobs < (1 << 20) ? n_jobs : (1 << 20);
    hipLaunchKernelGGL(k_contour_measures, dim3((unsigned)grid), dim3(kShapeLanes), 0, s, jobs, n_jobs,
                       xyz, theta, want2d, val, (long long*)idx);
    return hipGetLastError();
}

}  // namespace mm
