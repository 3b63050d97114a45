// mm_rim.cpp -- rim conditioning in front of the CCTA stitch (include/mm_ccta.h, "rim conditioning").  Reference:
// multimodars/ccta/stitching.py:484-1064 (_prepare_prox_dist_boundary_pts and its helpers).  The ring arithmetic touches
// a few hundred points and is host f64 here, unfused (-ffp-contract=off), like the seam in mm_stitch.cpp.  What the
// reference does over every vertex or face -- the {coordinate: index} dicts, the adjacency map behind the two vertex
// layers, the edge -> faces dict of the densification -- runs on the device (mm_rim_kernels.hip) on a mesh that stays
// resident from one upload to one download.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "../../include/mm_ccta.h"
#include "mm_stage.h"

namespace mm {
namespace {

constexpr int64_t kMaxRing = 1 << 20;      // ring points of one call

bool all_finite(const double* p, int64_t count)
{
    for (int64_t k = 0; k < count; ++k)
        if (!std::isfinite(p[k])) return false;
    return true;
}

// ---- the ring arithmetic (host) ------------------------------------------------------------------------------------------

// pts.mean(axis=0): the sequential sum of the rows divided by their number
void centroid_of(const double* p, int64_t n, double c[3])
{
    double s[3] = {0.0, 0.0, 0.0};
    for (int64_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) s[k] += p[3 * i + k];
    for (int k = 0; k < 3; ++k) c[k] = s[k] / (double)n;
}

inline double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
inline double norm3(const double* a) { return std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]); }

// _plane_normal_svd (:965-969) / :659-662: the centroid and the direction of least variance, as the eigenvector of the
// smallest eigenvalue of the 3 x 3 scatter matrix (cyclic Jacobi).  numpy takes the last right singular vector, whose
// sign LAPACK leaves open; here the component of largest magnitude is made positive.  Every use in the reference is
// indifferent to the sign: the projections multiply the normal by a distance that carries the same sign (:663-664,
// :782), _shift_plane_clear_of orients it along `outward` (:803-805), the angle takes |dot| (:974), the clamp multiplies
// it by sign-carrying factors (:996-1009), and the layer push subtracts (d n) with d = . n (:1051).
void fit_plane(const double* p, int64_t n, double c[3], double nrm[3])
{
    centroid_of(p, n, c);
    double a[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    for (int64_t i = 0; i < n; ++i) {
        const double d[3] = {p[3 * i] - c[0], p[3 * i + 1] - c[1], p[3 * i + 2] - c[2]};
        for (int r = 0; r < 3; ++r)
            for (int s = r; s < 3; ++s) a[r][s] += d[r] * d[s];
    }
    a[1][0] = a[0][1]; a[2][0] = a[0][2]; a[2][1] = a[1][2];
    for (int sweep = 0; sweep < 64; ++sweep) {
        if (std::fabs(a[0][1]) + std::fabs(a[0][2]) + std::fabs(a[1][2]) == 0.0) break;
        for (int x = 0; x < 2; ++x)
            for (int y = x + 1; y < 3; ++y) {
                const double g = 100.0 * std::fabs(a[x][y]);
                if (a[x][y] == 0.0) continue;
                if (sweep > 3 && std::fabs(a[x][x]) + g == std::fabs(a[x][x]) && std::fabs(a[y][y]) + g == std::fabs(a[y][y])) {
                    a[x][y] = a[y][x] = 0.0;
                    continue;
                }
                const double theta = (a[y][y] - a[x][x]) / (2.0 * a[x][y]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1.0));
                const double cs = 1.0 / std::sqrt(t * t + 1.0), sn = t * cs;
                const int z = 3 - x - y;
                const double axx = a[x][x], ayy = a[y][y], axy = a[x][y], axz = a[x][z], ayz = a[y][z];
                a[x][x] = axx - t * axy;
                a[y][y] = ayy + t * axy;
                a[x][y] = a[y][x] = 0.0;
                a[x][z] = a[z][x] = cs * axz - sn * ayz;
                a[y][z] = a[z][y] = sn * axz + cs * ayz;
                for (int r = 0; r < 3; ++r) {
                    const double vx = v[r][x], vy = v[r][y];
                    v[r][x] = cs * vx - sn * vy;
                    v[r][y] = sn * vx + cs * vy;
                }
            }
    }
    int m = 2;                                             // of equal eigenvalues the last axis, as numpy's Vt[-1] of zeros
    if (a[1][1] < a[m][m]) m = 1;
    if (a[0][0] < a[m][m]) m = 0;
    double e[3] = {v[0][m], v[1][m], v[2][m]};
    const double len = norm3(e);
    int big = 0;
    for (int k = 1; k < 3; ++k)
        if (std::fabs(e[k]) > std::fabs(e[big])) big = k;
    const double sgn = e[big] < 0.0 ? -1.0 : 1.0;
    for (int k = 0; k < 3; ++k) nrm[k] = sgn * (e[k] / len);
}

// :663-664 and :782: p - ((p - origin) . normal) normal
void project_onto(const double* p, int64_t n, const double o[3], const double nr[3], double* out)
{
    for (int64_t i = 0; i < n; ++i) {
        const double d[3] = {p[3 * i] - o[0], p[3 * i + 1] - o[1], p[3 * i + 2] - o[2]};
        const double dist = dot3(d, nr);
        for (int k = 0; k < 3; ++k) out[3 * i + k] = p[3 * i + k] - dist * nr[k];
    }
}

// _project_to_best_fit_plane (:648-665)
void project_best_fit(const double* p, int64_t n, double* out)
{
    if (n < 3) { std::memmove(out, p, (size_t)n * 24); return; }
    double c[3], nr[3];
    fit_plane(p, n, c, nr);
    project_onto(p, n, c, nr, out);
}

// _ring_calibre (:696-703)
double calibre(const double* p, int64_t n)
{
    double c[3], s = 0.0;
    centroid_of(p, n, c);
    for (int64_t i = 0; i < n; ++i) {
        const double d[3] = {p[3 * i] - c[0], p[3 * i + 1] - c[1], p[3 * i + 2] - c[2]};
        s += norm3(d);
    }
    return s / (double)n;
}

// _smooth_ring_preserving_size (:706-739) around _smooth_ring_laplacian (:668-693)
void smooth_preserving(const double* p, int64_t n, int64_t iterations, double alpha, double* out)
{
    if (n < 3) { std::memmove(out, p, (size_t)n * 24); return; }
    std::vector<double> cur(p, p + 3 * n), prev((size_t)(3 * n));
    const double before = calibre(p, n);
    for (int64_t it = 0; it < iterations; ++it) {
        prev.swap(cur);
        for (int64_t i = 0; i < n; ++i) {
            const int64_t a = (i + n - 1) % n, b = (i + 1) % n;
            for (int k = 0; k < 3; ++k) {
                const double avg = (prev[(size_t)(3 * a + k)] + prev[(size_t)(3 * b + k)]) / 2.0;
                cur[(size_t)(3 * i + k)] = alpha * prev[(size_t)(3 * i + k)] + (1.0 - alpha) * avg;
            }
        }
    }
    const double after = calibre(cur.data(), n);
    if (before <= 0.0 || after <= 0.0) { std::memcpy(out, cur.data(), (size_t)n * 24); return; }
    double c[3];
    centroid_of(cur.data(), n, c);
    const double scale = before / after;
    for (int64_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) out[3 * i + k] = c[k] + (cur[(size_t)(3 * i + k)] - c[k]) * scale;
}

// _redistribute_ring_evenly (:742-772); n_out < 0 is the reference's None.  Returns the number of points written.
int64_t redistribute(const double* p, int64_t n, int64_t n_out, double* out)
{
    const int64_t count = n_out < 0 ? n : n_out;
    if (n < 3 || count < 3) { std::memmove(out, p, (size_t)n * 24); return n; }
    std::vector<double> seg((size_t)n), cum((size_t)n + 1);
    cum[0] = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t j = (i + 1) % n;
        const double d[3] = {p[3 * j] - p[3 * i], p[3 * j + 1] - p[3 * i + 1], p[3 * j + 2] - p[3 * i + 2]};
        seg[(size_t)i] = norm3(d);
        cum[(size_t)i + 1] = cum[(size_t)i] + seg[(size_t)i];
    }
    const double perimeter = cum[(size_t)n];
    if (perimeter <= 0.0) { std::memmove(out, p, (size_t)n * 24); return n; }
    std::vector<double> res((size_t)(3 * count));
    const double step = perimeter / (double)count;                   // linspace(0, perimeter, count, endpoint=False)
    for (int64_t i = 0; i < count; ++i) {
        const double target = (double)i * step;
        // searchsorted(cum, target, side="right") - 1, clamped to the last segment
        int64_t k = (int64_t)(std::upper_bound(cum.begin(), cum.end(), target) - cum.begin()) - 1;
        if (k > n - 1) k = n - 1;
        const double span = seg[(size_t)k];
        const double frac = span <= 0.0 ? 0.0 : (target - cum[(size_t)k]) / span;
        const int64_t j = (k + 1) % n;
        for (int c = 0; c < 3; ++c) res[(size_t)(3 * i + c)] = p[3 * k + c] + frac * (p[3 * j + c] - p[3 * k + c]);
    }
    std::memcpy(out, res.data(), (size_t)count * 24);
    return count;
}

// _shift_plane_clear_of (:785-813); n >= 1
double shift_clear_of(const double o[3], const double nr[3], const double* pts, int64_t n, const double outward[3],
                      double overshoot, double so[3], double sn[3])
{
    const double len = norm3(nr);
    for (int k = 0; k < 3; ++k) sn[k] = nr[k] / len;
    if (dot3(sn, outward) < 0.0)
        for (int k = 0; k < 3; ++k) sn[k] = -sn[k];
    double worst = 0.0;
    for (int64_t i = 0; i < n; ++i) {
        const double d[3] = {pts[3 * i] - o[0], pts[3 * i + 1] - o[1], pts[3 * i + 2] - o[2]};
        const double s = dot3(d, sn);
        if (i == 0 || s > worst) worst = s;
    }
    if (worst <= -overshoot) {
        for (int k = 0; k < 3; ++k) so[k] = o[k];
        return 0.0;
    }
    const double shift = worst + overshoot;
    for (int k = 0; k < 3; ++k) so[k] = o[k] + shift * sn[k];
    return shift;
}

inline double np_sign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : 0.0); }

// _clamp_to_plane (:978-1011)
void clamp_to_plane(const double* p, int64_t n, const double o[3], const double nr[3], double overshoot, double* out)
{
    if (out != p) std::memmove(out, p, (size_t)n * 24);
    if (n == 0) return;
    std::vector<double> dist((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const double d[3] = {out[3 * i] - o[0], out[3 * i + 1] - o[1], out[3 * i + 2] - o[2]};
        dist[(size_t)i] = dot3(d, nr);
    }
    std::vector<double> sorted(dist);
    std::sort(sorted.begin(), sorted.end());
    const double median = n % 2 ? sorted[(size_t)(n / 2)] : (sorted[(size_t)(n / 2 - 1)] + sorted[(size_t)(n / 2)]) / 2.0;
    const double correct = np_sign(median);
    for (int64_t i = 0; i < n; ++i) {
        const double d = dist[(size_t)i];
        if (np_sign(d) != correct && d != 0.0)
            for (int k = 0; k < 3; ++k) out[3 * i + k] -= d * nr[k];
    }
    if (!(overshoot > 0.0)) return;
    for (int64_t i = 0; i < n; ++i) {
        const double d[3] = {out[3 * i] - o[0], out[3 * i + 1] - o[1], out[3 * i + 2] - o[2]};
        const double signed_dist = correct * dot3(d, nr);
        if (!(signed_dist < overshoot)) continue;
        const double w = (overshoot - signed_dist) * correct;
        for (int k = 0; k < 3; ++k) out[3 * i + k] += w * nr[k];
    }
}

// the counts of _densify_boundary (:862-892): 0 nothing to insert, 1 a plan, 2 the ring is above the target
int densify_plan(const double* p, int64_t n, int64_t target_n, int64_t* counts)
{
    for (int64_t i = 0; i < n; ++i) counts[i] = 0;
    const int64_t extra = target_n - n;
    if (n < 3 || extra <= 0) return extra < 0 ? 2 : 0;
    std::vector<double> len((size_t)n);
    std::vector<int64_t> order((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        const int64_t j = (i + 1) % n;
        const double d[3] = {p[3 * j] - p[3 * i], p[3 * j + 1] - p[3 * i + 1], p[3 * j + 2] - p[3 * i + 2]};
        len[(size_t)i] = norm3(d);
        order[(size_t)i] = i;
    }
    // sorted(..., reverse=True) is stable: equal lengths keep ring order
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return len[(size_t)a] > len[(size_t)b]; });
    for (int64_t i = 0; i < n; ++i) counts[i] = extra / n;
    for (int64_t k = 0; k < extra % n; ++k) ++counts[order[(size_t)k]];
    return 1;
}

// ---- the fans of _densify_boundary (:894-955), host ---------------------------------------------------------------------

struct Split {
    std::vector<double> new_v;            // the inserted points in ring-edge order, then one centroid per apex-less face
    std::vector<int32_t> fans;            // the faces that replace the touched ones, in ascending source-face order
    std::vector<int64_t> dense;           // the densified ring as vertex indices
    std::vector<double> dense_xyz;        // and as coordinates (all_vertices[...], :952-955)
    int64_t n_inserted = 0, n_centroid = 0;
};

// idx: the ring's n distinct vertices; rc: their coordinates as the mesh holds them; touched: (f, a, b, c) ascending in f
void build_fans(const int32_t* idx, const int64_t* counts, int64_t n, const double* rc, int64_t nv,
                const std::vector<int32_t>& touched, Split& out)
{
    std::vector<int64_t> off((size_t)n + 1, 0);
    for (int64_t i = 0; i < n; ++i) off[(size_t)i + 1] = off[(size_t)i] + counts[i];
    out.n_inserted = off[(size_t)n];
    out.new_v.resize((size_t)(3 * out.n_inserted));
    std::unordered_map<int32_t, int64_t> pos;
    for (int64_t i = 0; i < n; ++i) pos[idx[i]] = i;
    for (int64_t i = 0; i < n; ++i) {
        const int64_t j = (i + 1) % n, count = counts[i];
        out.dense.push_back(idx[i]);
        out.dense_xyz.insert(out.dense_xyz.end(), rc + 3 * i, rc + 3 * i + 3);
        for (int64_t k = 1; k <= count; ++k) {                        // pa + (k / (count + 1)) * (pb - pa), :902
            const double t = (double)k / (double)(count + 1);
            const int64_t at = off[(size_t)i] + k - 1;
            for (int c = 0; c < 3; ++c) out.new_v[(size_t)(3 * at + c)] = rc[3 * i + c] + t * (rc[3 * j + c] - rc[3 * i + c]);
            out.dense.push_back(nv + at);
            out.dense_xyz.insert(out.dense_xyz.end(), out.new_v.begin() + 3 * at, out.new_v.begin() + 3 * at + 3);
        }
    }
    auto coords = [&](int64_t v, double p[3]) {
        if (v >= nv) for (int c = 0; c < 3; ++c) p[c] = out.new_v[(size_t)(3 * (v - nv) + c)];
        else { const int64_t i = pos[(int32_t)v]; for (int c = 0; c < 3; ++c) p[c] = rc[3 * i + c]; }
    };
    // points_on (:909-915): the inserted ids along a -> b, reversed where the ring runs b -> a
    auto points_on = [&](int32_t a, int32_t b, std::vector<int64_t>& ids) {
        ids.clear();
        const auto ia = pos.find(a), ib = pos.find(b);
        if (ia == pos.end() || ib == pos.end()) return;
        const int64_t pa = ia->second, pb = ib->second;
        if ((pa + 1) % n == pb && counts[pa] > 0)
            for (int64_t k = 0; k < counts[pa]; ++k) ids.push_back(nv + off[(size_t)pa] + k);
        else if ((pb + 1) % n == pa && counts[pb] > 0)
            for (int64_t k = counts[pb] - 1; k >= 0; --k) ids.push_back(nv + off[(size_t)pb] + k);
    };
    std::vector<int64_t> poly, ids;
    for (size_t t = 0; t < touched.size() / 4; ++t) {
        const int32_t f[3] = {touched[4 * t + 1], touched[4 * t + 2], touched[4 * t + 3]};
        bool on_sub[3] = {false, false, false};
        poly.clear();
        for (int s = 0; s < 3; ++s) {
            const int32_t a = f[s], b = f[(s + 1) % 3];
            poly.push_back(a);
            points_on(a, b, ids);
            poly.insert(poly.end(), ids.begin(), ids.end());
            if (!ids.empty())
                for (int q = 0; q < 3; ++q)
                    if (f[q] == a || f[q] == b) on_sub[q] = true;
        }
        int apex = -1;
        for (int q = 0; q < 3 && apex < 0; ++q)
            if (!on_sub[q]) apex = q;
        const size_t m = poly.size();
        if (apex >= 0) {
            const size_t r = (size_t)(std::find(poly.begin(), poly.end(), (int64_t)f[apex]) - poly.begin());
            for (size_t i = 1; i + 1 < m; ++i) {
                out.fans.push_back((int32_t)poly[r]);
                out.fans.push_back((int32_t)poly[(r + i) % m]);
                out.fans.push_back((int32_t)poly[(r + i + 1) % m]);
            }
        } else {                                                       // all_vertices[poly].mean(axis=0), :944-950
            double s[3] = {0.0, 0.0, 0.0}, p[3];
            for (size_t i = 0; i < m; ++i) {
                coords(poly[i], p);
                for (int c = 0; c < 3; ++c) s[c] += p[c];
            }
            const int64_t cidx = nv + out.n_inserted + out.n_centroid++;
            for (int c = 0; c < 3; ++c) out.new_v.push_back(s[c] / (double)m);
            for (size_t i = 0; i < m; ++i) {
                out.fans.push_back((int32_t)cidx);
                out.fans.push_back((int32_t)poly[i]);
                out.fans.push_back((int32_t)poly[(i + 1) % m]);
            }
        }
    }
}

// ---- the resident mesh ---------------------------------------------------------------------------------------------------

struct Rim {
    Engine* e = nullptr;
    int64_t nv = 0, nf = 0, v_cap = 0, f_cap = 0, r_cap = 0;
    double* v = nullptr;
    int32_t *face = nullptr, *face2 = nullptr, *layer = nullptr, *fidx = nullptr, *list = nullptr;
    uint8_t* keep = nullptr;
    long long* tile = nullptr;
    unsigned long long* d_q = nullptr;
    int32_t *d_index = nullptr, *d_counts = nullptr;
    double* d_pts = nullptr;
    unsigned int* d_counter = nullptr;
    int64_t launches = 0, bytes_up = 0, bytes_down = 0;
    int64_t need_v = 0, need_f = 0;                                    // set where a stage passes v_cap / f_cap
};

int h2d(Rim& R, void* dst, const void* src, size_t bytes)
{
    if (bytes == 0) return MM_OK;
    MM_TRY_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, R.e->stream));
    MM_TRY_HIP(hipStreamSynchronize(R.e->stream));
    R.bytes_up += (int64_t)bytes;
    return MM_OK;
}

int d2h(Rim& R, void* dst, const void* src, size_t bytes)
{
    if (bytes == 0) return MM_OK;
    MM_TRY_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, R.e->stream));
    MM_TRY_HIP(hipStreamSynchronize(R.e->stream));
    R.bytes_down += (int64_t)bytes;
    return MM_OK;
}

// the mesh to the device: one copy of the vertices and one of the faces (int32) through the pinned buffer.  v_cap, f_cap:
// what the mesh may grow to; r_cap: the ring points of one stage.  faces == NULL: a stage that reads vertices only.
int rim_open(Rim& R, Engine* e, const double* v, int64_t nv, const int64_t* faces, int64_t nf, int64_t v_cap, int64_t f_cap,
             int64_t r_cap, const char* who)
{
    if (nv < 0 || nf < 0 || nv > kMaxIndex || nf > kMaxIndex || v_cap > kMaxIndex || f_cap > kMaxIndex || r_cap > kMaxRing ||
        (nv > 0 && !v) || (nf > 0 && !faces))
        return set_error(MM_ERR_INVALID, std::string(who) + ": bad arguments");
    if (const int bad = faces_in_range(faces, nf, nv, who)) return bad;
    R.e = e;
    R.nv = nv; R.nf = nf;
    R.v_cap = std::max(v_cap, nv); R.f_cap = std::max(f_cap, nf); R.r_cap = std::max<int64_t>(r_cap, 1);
    const size_t vc = (size_t)R.v_cap, fc = (size_t)R.f_cap, rc = (size_t)R.r_cap;
    int rc_ = carve_on(e, e->dev_pts, [&](Carve& c) {
        c.place(R.v, 3 * vc); c.place(R.face, 3 * fc); c.place(R.face2, 3 * fc); c.place(R.layer, vc);
        c.place(R.fidx, fc); c.place(R.list, 4 * fc); c.place(R.keep, fc);
        c.place(R.tile, trim_scan_tiles((long long)fc) + 1);
        c.place(R.d_q, 3 * rc); c.place(R.d_index, rc); c.place(R.d_counts, rc); c.place(R.d_pts, 3 * rc);
        c.place(R.d_counter, 2);                                       // the eight bytes the stages clear; one word is read
    });
    if (rc_) return rc_;
    if ((rc_ = e->ensure(e->host_pts, std::max((size_t)R.v_cap * 24, (size_t)R.f_cap * 12) + 256, true))) return rc_;
    unsigned char* hb = (unsigned char*)e->host_pts.p;
    if (nv > 0) {
        std::memcpy(hb, v, (size_t)nv * 24);
        if ((rc_ = h2d(R, R.v, hb, (size_t)nv * 24))) return rc_;
    }
    if (nf > 0) {
        int32_t* hf = (int32_t*)hb;
        narrow_faces(hf, faces, 3 * nf);
        if ((rc_ = h2d(R, R.face, hb, (size_t)nf * 12))) return rc_;
    }
    return MM_OK;
}

// the mesh back: the other copy of the call
int rim_close(Rim& R, double* out_v, int64_t* out_f)
{
    unsigned char* hb = (unsigned char*)R.e->host_pts.p;
    int rc;
    if (R.nv > 0 && out_v) {
        if ((rc = d2h(R, hb, R.v, (size_t)R.nv * 24))) return rc;
        std::memcpy(out_v, hb, (size_t)R.nv * 24);
    }
    if (R.nf > 0 && out_f) {
        if ((rc = d2h(R, hb, R.face, (size_t)R.nf * 12))) return rc;
        const int32_t* hf = (const int32_t*)hb;
        widen_faces(out_f, hf, 3 * R.nf);
    }
    return MM_OK;
}

// coord_to_idx.get(tuple(p)) for every p (:826-830, :873-874): index[k] = the last vertex equal to point k by value
int rim_locate(Rim& R, const double* pts, int64_t r, std::vector<int32_t>& index)
{
    index.assign((size_t)r, -1);
    if (r == 0 || R.nv == 0) return MM_OK;
    if (r > R.r_cap) return set_error(MM_ERR_INVALID, "rim: more ring points than the call was sized for");
    std::vector<unsigned long long> q((size_t)(3 * r));
    for (int64_t k = 0; k < 3 * r; ++k) {
        const double x = pts[k] == 0.0 ? 0.0 : pts[k];               // -0.0 == 0.0, as dict keys compare
        std::memcpy(&q[(size_t)k], &x, 8);
    }
    int rc;
    if ((rc = h2d(R, R.d_q, q.data(), (size_t)r * 24))) return rc;
    MM_TRY_HIP(hipMemsetAsync(R.d_index, 0xFF, (size_t)r * 4, R.e->stream));
    MM_TRY_HIP(launch_rim_locate(R.v, R.nv, R.d_q, (int)r, R.d_index, R.e->stream));
    ++R.launches;
    return d2h(R, index.data(), R.d_index, (size_t)r * 4);
}

// _write_ring_to_mesh (:816-834) with the located indices; moved: the distinct vertices written, ascending
int rim_write(Rim& R, const std::vector<int32_t>& index, const double* new_pts, std::vector<int32_t>& moved)
{
    const int64_t r = (int64_t)index.size();
    std::vector<std::pair<int32_t, int64_t>> by((size_t)r);
    for (int64_t i = 0; i < r; ++i) by[(size_t)i] = {index[(size_t)i], i};
    std::sort(by.begin(), by.end());
    moved.clear();
    for (int64_t k = 0; k < r; ++k) {
        if (by[(size_t)k].first < 0) continue;
        if (k > 0 && by[(size_t)k].first == by[(size_t)k - 1].first) {
            // the reference keeps the last of two targets for one vertex; a parallel scatter has no last: rejected
            if (std::memcmp(new_pts + 3 * by[(size_t)k].second, new_pts + 3 * by[(size_t)k - 1].second, 24) != 0)
                return set_error(MM_ERR_INVALID, "rim: two ring points with different targets sit on one mesh vertex");
            continue;
        }
        moved.push_back(by[(size_t)k].first);
    }
    if (moved.empty()) return MM_OK;
    int rc;
    if ((rc = h2d(R, R.d_index, index.data(), (size_t)r * 4))) return rc;
    if ((rc = h2d(R, R.d_pts, new_pts, (size_t)r * 24))) return rc;
    MM_TRY_HIP(launch_rim_write(R.d_index, R.d_pts, (int)r, R.v, R.e->stream));
    ++R.launches;
    return MM_OK;
}

// _enforce_layer_gap_from_plane (:1014-1064): counts[k - 1] = the vertices of layer k, for the rings that ran
int rim_layer_push(Rim& R, const std::vector<int32_t>& seeds, const double o[3], const double nr[3], double step,
                   int64_t n_rings, std::vector<int64_t>& counts)
{
    counts.clear();
    if (R.nv == 0) return MM_OK;
    MM_TRY_HIP(hipMemsetAsync(R.layer, 0xFF, (size_t)R.nv * 4, R.e->stream));
    if (seeds.empty() || n_rings <= 0) return MM_OK;
    if ((int64_t)seeds.size() > R.r_cap) return set_error(MM_ERR_INVALID, "rim: more seeds than the call was sized for");
    int rc;
    if ((rc = h2d(R, R.d_index, seeds.data(), seeds.size() * 4))) return rc;
    MM_TRY_HIP(launch_rim_mark(R.d_index, (int)seeds.size(), 0, R.layer, R.e->stream));
    ++R.launches;
    int64_t total = 0;
    for (int64_t k = 1; k <= n_rings && R.nf > 0; ++k) {
        MM_TRY_HIP(hipMemsetAsync(R.d_counter, 0, 8, R.e->stream));
        MM_TRY_HIP(launch_rim_layer(R.face, R.nf, R.layer, (int32_t)k, R.d_counter, R.e->stream));
        ++R.launches;
        unsigned int c = 0;
        if ((rc = d2h(R, &c, R.d_counter, 4))) return rc;
        counts.push_back((int64_t)c);
        total += c;
        if (c == 0) break;                                             // the frontier is empty (:1061)
    }
    if (total > 0) {
        MM_TRY_HIP(launch_rim_push(R.v, R.nv, R.layer, o, nr, step, R.e->stream));
        ++R.launches;
    }
    return MM_OK;
}

// the mesh side of _densify_boundary (:873-962) for a ring located on the mesh.  MM_ERR_TOO_LARGE where the result
// passes v_cap / f_cap: need_v / need_f then hold its size and the mesh is left as it was.
int rim_split(Rim& R, const std::vector<int32_t>& idx, const int64_t* counts, Split& sp, int64_t* n_fanned)
{
    const int64_t n = (int64_t)idx.size();
    *n_fanned = 0;
    {
        std::vector<int32_t> s(idx);
        std::sort(s.begin(), s.end());
        if (std::adjacent_find(s.begin(), s.end()) != s.end())
            return set_error(MM_ERR_INVALID, "rim: the ring names one mesh vertex twice");
    }
    if (n > R.r_cap) return set_error(MM_ERR_INVALID, "rim: more ring points than the call was sized for");
    std::vector<int32_t> c32((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        if (counts[i] < 0 || counts[i] > kMaxRing) return set_error(MM_ERR_INVALID, "rim: insert count out of range");
        c32[(size_t)i] = (int32_t)counts[i];
    }
    int rc;
    std::vector<double> rcoord((size_t)(3 * n));
    MM_TRY_HIP(hipMemsetAsync(R.layer, 0xFF, (size_t)R.nv * 4, R.e->stream));      // pos[v]
    if ((rc = h2d(R, R.d_index, idx.data(), (size_t)n * 4))) return rc;
    if ((rc = h2d(R, R.d_counts, c32.data(), (size_t)n * 4))) return rc;
    MM_TRY_HIP(launch_rim_mark(R.d_index, (int)n, 1, R.layer, R.e->stream));
    MM_TRY_HIP(launch_rim_gather(R.v, R.d_index, (int)n, R.d_pts, R.e->stream));
    R.launches += 2;
    if ((rc = d2h(R, rcoord.data(), R.d_pts, (size_t)n * 24))) return rc;
    std::vector<int32_t> touched;
    if (R.nf > 0) {
        MM_TRY_HIP(hipMemsetAsync(R.d_counter, 0, 8, R.e->stream));
        MM_TRY_HIP(launch_rim_edge_faces(R.face, R.nf, R.layer, R.d_counts, (int)n, R.keep, R.list, (unsigned int)R.nf,
                                         R.d_counter, R.e->stream));
        ++R.launches;
        unsigned int t = 0;
        if ((rc = d2h(R, &t, R.d_counter, 4))) return rc;
        if ((int64_t)t > R.nf) return set_error(MM_ERR_HIP, "rim: touched face count out of range");
        touched.resize((size_t)t * 4);
        if ((rc = d2h(R, touched.data(), R.list, (size_t)t * 16))) return rc;
        // the list comes in no order: ascending face index is the rule (the reference walks a Python set)
        std::vector<size_t> ord(t);
        for (size_t k = 0; k < t; ++k) ord[k] = k;
        std::sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return touched[4 * a] < touched[4 * b]; });
        std::vector<int32_t> sorted((size_t)t * 4);
        for (size_t k = 0; k < t; ++k) std::memcpy(&sorted[4 * k], &touched[4 * ord[k]], 16);
        touched.swap(sorted);
    }
    const int64_t t = (int64_t)touched.size() / 4;
    build_fans(idx.data(), counts, n, rcoord.data(), R.nv, touched, sp);
    const int64_t n_new_v = (int64_t)sp.new_v.size() / 3, n_fan = (int64_t)sp.fans.size() / 3;
    const int64_t nv2 = R.nv + n_new_v, nf2 = R.nf - t + n_fan;
    if (nv2 > R.v_cap || nf2 > R.f_cap) {
        R.need_v = nv2; R.need_f = nf2;
        return set_error(MM_ERR_TOO_LARGE, "rim: the densified mesh passes vert_cap / face_cap (the report holds the sizes)");
    }
    if ((rc = h2d(R, R.v + 3 * R.nv, sp.new_v.data(), (size_t)n_new_v * 24))) return rc;
    if (t > 0) {                                                       // the untouched faces in input order, then the fans
        MM_TRY_HIP(launch_trim_scan(R.keep, R.nf, R.tile, R.fidx, R.e->stream));
        MM_TRY_HIP(launch_rim_face_gather(R.face, R.nf, R.fidx, R.face2, R.e->stream));
        R.launches += 4;
        if ((rc = h2d(R, R.face2 + 3 * (R.nf - t), sp.fans.data(), (size_t)n_fan * 12))) return rc;
        std::swap(R.face, R.face2);
    }
    R.nv = nv2; R.nf = nf2;
    *n_fanned = t;
    return MM_OK;
}

}  // namespace
}  // namespace mm

using namespace mm;

extern "C" {

int mm_ring_fit_plane(const double* ring_xyz, int64_t n, double origin[3], double normal[3])
{
    if (n < 1 || !ring_xyz || !origin || !normal || !all_finite(ring_xyz, 3 * n))
        return set_error(MM_ERR_INVALID, "mm_ring_fit_plane: bad arguments");
    fit_plane(ring_xyz, n, origin, normal);
    return MM_OK;
}

int mm_ring_project_to_plane(const double* ring_xyz, int64_t n, const double* origin, const double* normal, double* out)
{
    if (n < 0 || (n > 0 && (!ring_xyz || !out)) || (origin == nullptr) != (normal == nullptr) || !all_finite(ring_xyz, 3 * n) ||
        (origin && (!all_finite(origin, 3) || !all_finite(normal, 3))))
        return set_error(MM_ERR_INVALID, "mm_ring_project_to_plane: bad arguments");
    if (origin) project_onto(ring_xyz, n, origin, normal, out);
    else project_best_fit(ring_xyz, n, out);
    return MM_OK;
}

int mm_ring_smooth_preserving_size(const double* ring_xyz, int64_t n, int64_t iterations, double alpha, double* out)
{
    if (n < 0 || iterations < 0 || (n > 0 && (!ring_xyz || !out)) || !std::isfinite(alpha) || !all_finite(ring_xyz, 3 * n))
        return set_error(MM_ERR_INVALID, "mm_ring_smooth_preserving_size: bad arguments");
    smooth_preserving(ring_xyz, n, iterations, alpha, out);
    return MM_OK;
}

int64_t mm_ring_redistribute(const double* ring_xyz, int64_t n, int64_t n_out, double* out)
{
    if (n < 0 || n_out < -1 || n_out > kMaxRing || (n > 0 && (!ring_xyz || !out)) || !all_finite(ring_xyz, 3 * n))
        return set_error(MM_ERR_INVALID, "mm_ring_redistribute: bad arguments");
    return redistribute(ring_xyz, n, n_out, out);
}

int mm_plane_shift_clear_of(const double origin[3], const double normal[3], const double* pts_xyz, int64_t n,
                            const double outward[3], double overshoot, double out_origin[3], double out_normal[3],
                            double* moved)
{
    if (n < 1 || !origin || !normal || !pts_xyz || !outward || !out_origin || !out_normal || !moved ||
        !std::isfinite(overshoot) || !all_finite(origin, 3) || !all_finite(normal, 3) || !all_finite(outward, 3) ||
        !all_finite(pts_xyz, 3 * n) || norm3(normal) == 0.0)
        return set_error(MM_ERR_INVALID, "mm_plane_shift_clear_of: bad arguments");
    *moved = shift_clear_of(origin, normal, pts_xyz, n, outward, overshoot, out_origin, out_normal);
    return MM_OK;
}

int mm_ring_clamp_to_plane(const double* ring_xyz, int64_t n, const double origin[3], const double normal[3],
                           double overshoot, double* out)
{
    if (n < 0 || (n > 0 && (!ring_xyz || !out)) || !origin || !normal || !std::isfinite(overshoot) ||
        !all_finite(origin, 3) || !all_finite(normal, 3) || !all_finite(ring_xyz, 3 * n))
        return set_error(MM_ERR_INVALID, "mm_ring_clamp_to_plane: bad arguments");
    clamp_to_plane(ring_xyz, n, origin, normal, overshoot, out);
    return MM_OK;
}

int mm_ring_densify_plan(const double* ring_xyz, int64_t n, int64_t target_n, int64_t* counts)
{
    if (n < 0 || target_n < 0 || target_n > kMaxRing || (n > 0 && (!ring_xyz || !counts)) || !all_finite(ring_xyz, 3 * n))
        return set_error(MM_ERR_INVALID, "mm_ring_densify_plan: bad arguments");
    return densify_plan(ring_xyz, n, target_n, counts);
}

int mm_rim_locate_chunk_points(void) { return rim_locate_chunk_points(); }

int mm_mesh_locate_points(mm_engine* h, const double* vertices_xyz, int64_t nv, const double* pts_xyz, int64_t r,
                          int64_t* index)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (r < 0 || r > kMaxRing || (r > 0 && (!pts_xyz || !index)))
        return set_error(MM_ERR_INVALID, "mm_mesh_locate_points: bad arguments");
    Rim R;
    if ((rc = rim_open(R, e, vertices_xyz, nv, nullptr, 0, nv, 0, r, "mm_mesh_locate_points"))) return rc;
    std::vector<int32_t> idx;
    if ((rc = rim_locate(R, pts_xyz, r, idx))) return rc;
    for (int64_t k = 0; k < r; ++k) index[k] = idx[(size_t)k];
    return MM_OK;
}

int mm_mesh_layer_push(mm_engine* h, const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf,
                       const int64_t* seeds, int64_t ns, const double origin[3], const double normal[3], double layer_step,
                       int64_t n_rings, double* out_vertices, int32_t* out_layer, int64_t* info)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (ns < 0 || ns > kMaxRing || n_rings < 0 || n_rings > kMaxIndex || (ns > 0 && !seeds) || !origin || !normal || !info ||
        (nv > 0 && (!out_vertices || !out_layer)) || !all_finite(origin, 3) || !all_finite(normal, 3) || !std::isfinite(layer_step))
        return set_error(MM_ERR_INVALID, "mm_mesh_layer_push: bad arguments");
    std::vector<int32_t> s32;
    for (int64_t k = 0; k < ns; ++k) {
        if (seeds[k] < 0 || seeds[k] >= nv) return set_error(MM_ERR_INVALID, "mm_mesh_layer_push: seed out of range");
        s32.push_back((int32_t)seeds[k]);
    }
    Rim R;
    if ((rc = rim_open(R, e, vertices_xyz, nv, faces, nf, nv, nf, ns, "mm_mesh_layer_push"))) return rc;
    std::vector<int64_t> counts;
    if ((rc = rim_layer_push(R, s32, origin, normal, layer_step, n_rings, counts))) return rc;
    if ((rc = rim_close(R, out_vertices, nullptr))) return rc;
    if (nv > 0 && (rc = d2h(R, out_layer, R.layer, (size_t)nv * 4))) return rc;
    info[0] = R.launches;
    info[1] = (int64_t)counts.size();
    info[2] = 0;
    for (int64_t c : counts) info[2] += c;
    return MM_OK;
}

int mm_mesh_split_rim_edges(mm_engine* h, const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf,
                            const int64_t* ring_idx, int64_t n, const int64_t* counts, int64_t vert_cap, int64_t face_cap,
                            double* out_vertices, int64_t* out_faces, int64_t* out_ring_idx, int64_t* info)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (n < 3 || n > kMaxRing || !ring_idx || !counts || !info || vert_cap < 0 || face_cap < 0 || !out_ring_idx ||
        (vert_cap > 0 && !out_vertices) || (face_cap > 0 && !out_faces))
        return set_error(MM_ERR_INVALID, "mm_mesh_split_rim_edges: bad arguments");
    std::vector<int32_t> idx;
    for (int64_t k = 0; k < n; ++k) {
        if (ring_idx[k] < 0 || ring_idx[k] >= nv) return set_error(MM_ERR_INVALID, "mm_mesh_split_rim_edges: ring vertex out of range");
        idx.push_back((int32_t)ring_idx[k]);
    }
    std::memset(info, 0, 6 * sizeof(int64_t));
    Rim R;
    if ((rc = rim_open(R, e, vertices_xyz, nv, faces, nf, vert_cap, face_cap, n, "mm_mesh_split_rim_edges"))) return rc;
    if (vert_cap < nv || face_cap < nf) {                             // rim_open widened them to hold the input
        R.v_cap = nv; R.f_cap = nf;
    }
    Split sp;
    int64_t n_fanned = 0;
    rc = rim_split(R, idx, counts, sp, &n_fanned);
    info[5] = R.launches;
    if (rc == MM_ERR_TOO_LARGE) { info[0] = R.need_v; info[1] = R.need_f; }
    if (rc) return rc;
    info[0] = R.nv; info[1] = R.nf; info[2] = sp.n_inserted; info[3] = n_fanned; info[4] = sp.n_centroid;
    if (vert_cap < R.nv || face_cap < R.nf)
        return set_error(MM_ERR_TOO_LARGE, "mm_mesh_split_rim_edges: vert_cap / face_cap too small (info holds the sizes)");
    if ((rc = rim_close(R, out_vertices, out_faces))) return rc;
    for (size_t k = 0; k < sp.dense.size(); ++k) out_ring_idx[k] = sp.dense[k];
    return MM_OK;
}

int mm_condition_rims(mm_engine* h, const double* vertices_xyz, int64_t nv, const int64_t* faces, int64_t nf,
                      const double* prox_ring, int64_t n_prox, const double* dist_ring, int64_t n_dist,
                      const double* iv_frame, int64_t n_iv, const double prox_centroid[3], const double* prox_outward,
                      const double* aorta_xyz, int64_t na, const mm_rim_params* params, double* out_vertices,
                      int64_t* out_faces, double* out_prox, double* out_dist, mm_rim_report* report)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    if (!params || !report || n_prox < 0 || n_dist < 0 || n_iv < 0 || na < 0 || n_prox > kMaxRing || n_dist > kMaxRing ||
        (n_prox > 0 && !prox_ring) || (n_dist > 0 && !dist_ring) || (n_iv > 0 && !iv_frame) || (na > 0 && !aorta_xyz) ||
        !prox_centroid)
        return set_error(MM_ERR_INVALID, "mm_condition_rims: bad arguments");
    const mm_rim_params& P = *params;
    if (P.target_n < 0 || P.target_n > kMaxRing || P.smooth_iterations < 0 || P.n_rings < 0 || P.vert_cap < 0 ||
        P.face_cap < 0 || P.ring_cap < 0 || (P.vert_cap > 0 && !out_vertices) || (P.face_cap > 0 && !out_faces) ||
        (P.ring_cap > 0 && (!out_prox || !out_dist)) || !std::isfinite(P.smooth_alpha) ||
        !std::isfinite(P.angle_threshold_deg) || !std::isfinite(P.clamp_overshoot) || !std::isfinite(P.layer_step_mm))
        return set_error(MM_ERR_INVALID, "mm_condition_rims: bad parameters");
    if (!all_finite(prox_ring, 3 * n_prox) || !all_finite(dist_ring, 3 * n_dist) || !all_finite(iv_frame, 3 * n_iv) ||
        !all_finite(aorta_xyz, 3 * na) || !all_finite(prox_centroid, 3) || (prox_outward && !all_finite(prox_outward, 3)))
        return set_error(MM_ERR_INVALID, "mm_condition_rims: non-finite ring, frame or direction");
    std::memset(report, 0, sizeof(*report));
    const int64_t r_cap = std::max(std::max(n_prox, n_dist), P.target_n);
    Rim R;
    if ((rc = rim_open(R, e, vertices_xyz, nv, faces, nf, P.vert_cap, P.face_cap, r_cap, "mm_condition_rims"))) return rc;

    // :529-536: flatten, smooth, respace, write back -- the proximal rim, then the distal one
    std::vector<double> ring[2];
    std::vector<int32_t> index, moved;
    const double* src[2] = {prox_ring, dist_ring};
    const int64_t len[2] = {n_prox, n_dist};
    for (int s = 0; s < 2; ++s) {
        const int64_t n = len[s];
        std::vector<double> a((size_t)(3 * n)), b((size_t)(3 * n));
        ring[s].resize((size_t)(3 * n));
        project_best_fit(src[s], n, a.data());
        smooth_preserving(a.data(), n, P.smooth_iterations, P.smooth_alpha, b.data());
        redistribute(b.data(), n, -1, ring[s].data());
        if ((rc = rim_locate(R, src[s], n, index))) return rc;
        if ((rc = rim_write(R, index, ring[s].data(), moved))) return rc;
        (s == 0 ? report->n_moved_prox : report->n_moved_dist) = (int64_t)moved.size();
    }

    // _condition_ostium_ring (:582-645)
    if (P.proximal_is_ostium && n_iv > 0 && n_prox >= 3) {
        const int64_t n = n_prox;
        const std::vector<double> original(ring[0]);
        std::vector<double>& rg = ring[0];
        double c[3], nr[3], dir[3];
        bool have_dir = false;
        centroid_of(rg.data(), n, c);
        if (na > 0) {                                                  // _toward_aorta (:559-579)
            double ac[3];
            centroid_of(aorta_xyz, na, ac);
            for (int k = 0; k < 3; ++k) dir[k] = ac[k] - c[k];
            have_dir = dir[0] != 0.0 || dir[1] != 0.0 || dir[2] != 0.0;
        }
        if (!have_dir && prox_outward && (prox_outward[0] != 0.0 || prox_outward[1] != 0.0 || prox_outward[2] != 0.0)) {
            for (int k = 0; k < 3; ++k) dir[k] = prox_outward[k];
            have_dir = true;
        }
        if (have_dir) {
            double so[3], sn[3];
            fit_plane(rg.data(), n, c, nr);
            const double shift = shift_clear_of(c, nr, iv_frame, n_iv, dir, P.clamp_overshoot, so, sn);
            if (shift > 0.0) {
                report->plane_shift_mm = shift;
                std::vector<double> t(rg);
                project_onto(t.data(), n, so, sn, rg.data());
            }
        }
        double ivc[3], ivn[3];
        fit_plane(iv_frame, n_iv, ivc, ivn);
        fit_plane(rg.data(), n, c, nr);
        double cosine = std::fabs(dot3(nr, ivn));                      // _angle_between_planes_deg (:972-975)
        cosine = cosine > 1.0 ? 1.0 : cosine;
        report->plane_angle_deg = std::acos(cosine) * (180.0 / M_PI);
        if (report->plane_angle_deg >= P.angle_threshold_deg) {
            clamp_to_plane(rg.data(), n, prox_centroid, ivn, P.clamp_overshoot, rg.data());
            report->clamped = 1;
        }
        if ((rc = rim_locate(R, original.data(), n, index))) return rc;
        if ((rc = rim_write(R, index, rg.data(), moved))) return rc;
        report->n_moved_ostium = (int64_t)moved.size();
        if (report->clamped && !moved.empty()) {
            std::vector<int64_t> counts;
            if ((rc = rim_layer_push(R, moved, prox_centroid, ivn, P.layer_step_mm, P.n_rings, counts))) return rc;
            for (size_t k = 0; k < counts.size() && k < 2; ++k) report->n_layer_vertices[k] = counts[k];
        }
    }

    // _densify_boundary (:837-962), last: the inserted points lie between the final positions
    for (int s = 0; s < 2 && P.target_n > 0; ++s) {
        const int64_t n = len[s];
        std::vector<int64_t> counts((size_t)n);
        const int plan = densify_plan(ring[s].data(), n, P.target_n, counts.data());
        if (plan == 2) report->ring_over_target[s] = 1;
        if (plan != 1) continue;
        if ((rc = rim_locate(R, ring[s].data(), n, index))) return rc;
        if (std::find(index.begin(), index.end(), -1) != index.end()) { report->ring_off_mesh[s] = 1; continue; }
        Split sp;
        int64_t n_fanned = 0;
        rc = rim_split(R, index, counts.data(), sp, &n_fanned);
        if (rc == MM_ERR_TOO_LARGE) {
            // what is known: this result, and for a ring still to come the bound of a rim whose edges have one owner
            report->n_vertices = R.need_v;
            report->n_faces = R.need_f;
            if (s == 0 && n_dist >= 3 && P.target_n > n_dist) {
                report->n_vertices += P.target_n;
                report->n_faces += 2 * P.target_n;
            }
            report->n_launches = R.launches;
        }
        if (rc) return rc;
        (s == 0 ? report->n_inserted_prox : report->n_inserted_dist) = sp.n_inserted;
        report->n_fanned_faces += n_fanned;
        report->n_centroid_fans += sp.n_centroid;
        ring[s].swap(sp.dense_xyz);                                   // walk order, the mesh's own coordinates
    }

    report->n_vertices = R.nv;
    report->n_faces = R.nf;
    report->n_prox = (int64_t)ring[0].size() / 3;
    report->n_dist = (int64_t)ring[1].size() / 3;
    report->n_launches = R.launches;
    if (P.vert_cap < R.nv || P.face_cap < R.nf || P.ring_cap < report->n_prox || P.ring_cap < report->n_dist)
        return set_error(MM_ERR_TOO_LARGE, "mm_condition_rims: vert_cap / face_cap / ring_cap too small (the report holds the sizes)");
    if ((rc = rim_close(R, out_vertices, out_faces))) return rc;
    if (!ring[0].empty()) std::memcpy(out_prox, ring[0].data(), ring[0].size() * 8);
    if (!ring[1].empty()) std::memcpy(out_dist, ring[1].data(), ring[1].size() * 8);
    report->bytes_uploaded = R.bytes_up;
    report->bytes_downloaded = R.bytes_down;
    return MM_OK;
}

}  // extern "C"
