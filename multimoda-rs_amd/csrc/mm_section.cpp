// mm_section.cpp -- mesh cross-sections (include/mm_ccta.h, "mesh cross-sections"): the exact intersection of a triangle
// mesh with a stack of planes, as contours with their measures.  Nothing in the reference does this; its discretisation
// gives vertices to slices (mm_discretize.cpp).  The host checks the arguments, stages the faces in slab order
// (mm_prune.h), keeps for every chunk the planes whose height changes sign over the chunk's box (rule 8) and cuts each
// list into runs; every (plane, face) pair of an item is tested on the device (mm_section_kernels.hip), which returns
// one segment per crossed face.  The host sorts the segments by (plane, face), chains them into contours (rule 5),
// measures them (rule 6) and selects the loop around each origin (rule 7).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/mm_ccta.h"
#include "mm_section_device.h"
#include "mm_tri_plan.h"

using namespace mm;
using section::Plane;
using section::Segment;

namespace {

struct SectionPlan {
    int ch = section::kChunk, run = section::kPlaneRun;
    std::vector<int32_t> order;        // staged face j is face order[j]
    std::vector<uint8_t> skipped;      // per staged face: a repeated index
    std::vector<Box3> cbox;            // the box of every chunk's corners
    std::vector<int32_t> plane_list;   // per chunk, ascending, the planes that pass rule 8; chunk after chunk
    std::vector<int32_t> items;        // 4 each: chunk, first entry in plane_list, planes (at most `run`), 0
    int64_t n_pairs = 0, pairs_total = 0, face_tests = 0, n_skipped = 0;
    int64_t n_items() const { return (int64_t)items.size() / 4; }
};

int check_planes(const double* origins, const double* normals, int64_t n_planes, const char* who)
{
    if (n_planes < 0 || (n_planes > 0 && (!origins || !normals)))
        return set_error(MM_ERR_INVALID, std::string(who) + ": bad arguments");
    if (n_planes > kMaxIndex) return set_error(MM_ERR_INVALID, std::string(who) + ": n_planes must stay below 2^31");
    for (int64_t k = 0; k < 3 * n_planes; ++k)
        if (!std::isfinite(origins[k])) return set_error(MM_ERR_INVALID, std::string(who) + ": non-finite plane origin");
    for (int64_t p = 0; p < n_planes; ++p) {
        const double* n = normals + 3 * p;
        if (!std::isfinite(n[0]) || !std::isfinite(n[1]) || !std::isfinite(n[2]))
            return set_error(MM_ERR_INVALID, std::string(who) + ": non-finite plane normal");
        if (n[0] == 0.0 && n[1] == 0.0 && n[2] == 0.0) return set_error(MM_ERR_INVALID, std::string(who) + ": zero plane normal");
    }
    return MM_OK;
}

Plane plane_of(const double* origins, const double* normals, int64_t p)
{
    return Plane{origins[3 * p], origins[3 * p + 1], origins[3 * p + 2], normals[3 * p], normals[3 * p + 1], normals[3 * p + 2]};
}

// Arguments checked by plan_args and check_planes.
int build_section_plan(const double* v, const int64_t* f, int64_t nf, const double* origins, const double* normals,
                       int64_t n_planes, const char* who, SectionPlan& pl)
{
    TraceTimer t_order("section: slab order");
    Box3 all;
    for (int64_t k = 0; k < 3 * nf; ++k) all.add(v + 3 * f[k]);
    const int ax = all.longest_axis();
    std::vector<double> key((size_t)nf);
    for (int64_t i = 0; i < nf; ++i) key[(size_t)i] = (v[3 * f[3 * i] + ax] + v[3 * f[3 * i + 1] + ax]) + v[3 * f[3 * i + 2] + ax];
    slab_permutation(key, pl.order);
    const int64_t nch = (nf + pl.ch - 1) / pl.ch;
    pl.skipped.resize((size_t)nf);
    pl.cbox.assign((size_t)nch, Box3{});
    pl.n_skipped = 0;
    for (int64_t j = 0; j < nf; ++j) {
        const int64_t* t = f + 3 * (int64_t)pl.order[(size_t)j];
        pl.skipped[(size_t)j] = t[0] == t[1] || t[1] == t[2] || t[0] == t[2];
        pl.n_skipped += pl.skipped[(size_t)j];
        for (int k = 0; k < 3; ++k) pl.cbox[(size_t)(j / pl.ch)].add(v + 3 * t[k]);
    }
    t_order.stop();
    TraceTimer t_items("section: items");
    pl.plane_list.clear();
    pl.items.clear();
    pl.n_pairs = pl.face_tests = 0;
    pl.pairs_total = nch * n_planes;
    std::vector<Plane> planes((size_t)n_planes);
    for (int64_t p = 0; p < n_planes; ++p) planes[(size_t)p] = plane_of(origins, normals, p);
    for (int64_t c = 0; c < nch; ++c) {
        const Box3& b = pl.cbox[(size_t)c];
        const int64_t first = (int64_t)pl.plane_list.size();
        for (int64_t p = 0; p < n_planes; ++p) {
            double h_min, h_max;
            section::box_heights(planes[(size_t)p], b.lo, b.hi, h_min, h_max);
            if (section::box_takes_part(h_min, h_max)) pl.plane_list.push_back((int32_t)p);
        }
        const int64_t n = (int64_t)pl.plane_list.size() - first;
        if ((int64_t)pl.plane_list.size() > kMaxIndex)
            return set_error(MM_ERR_TOO_LARGE, std::string(who) + ": more than 2^31 - 1 (plane, chunk) pairs");
        pl.n_pairs += n;
        pl.face_tests += n * std::min<int64_t>(pl.ch, nf - c * pl.ch);
        for (int64_t r = 0; r < n; r += pl.run) {
            const int32_t it[4] = {(int32_t)c, (int32_t)(first + r), (int32_t)std::min<int64_t>(pl.run, n - r), 0};
            pl.items.insert(pl.items.end(), it, it + 4);
        }
    }
    return MM_OK;
}

// 12 doubles a face: a, b, c as x y z w; a.w = index 0 | index 1 << 32, b.w = index 2 | original face << 32, c.w = skipped
void stage_section_records(const SectionPlan& pl, const double* v, const int64_t* f, int64_t nf, double* t)
{
    for (int64_t j = 0; j < nf; ++j, t += 12) {
        const int64_t orig = pl.order[(size_t)j];
        const int64_t* tri = f + 3 * orig;
        const unsigned long long w[3] = {(unsigned long long)(uint32_t)tri[0] | (unsigned long long)(uint32_t)tri[1] << 32,
                                         (unsigned long long)(uint32_t)tri[2] | (unsigned long long)orig << 32,
                                         pl.skipped[(size_t)j] ? 1ull : 0ull};
        for (int k = 0; k < 3; ++k) {
            std::memcpy(t + 4 * k, v + 3 * tri[k], 24);
            std::memcpy(t + 4 * k + 3, &w[k], 8);
        }
    }
}

// the items of a plan on the host, with the arithmetic the kernel runs: the test hook's cut
void cut_on_host(const SectionPlan& pl, const double* v, const int64_t* f, int64_t nf, const double* origins,
                 const double* normals, std::vector<Segment>& out)
{
    for (int64_t w = 0; w < pl.n_items(); ++w) {
        const int32_t* it = pl.items.data() + 4 * w;
        for (int64_t j = (int64_t)it[0] * pl.ch; j < std::min<int64_t>(nf, ((int64_t)it[0] + 1) * pl.ch); ++j) {
            if (pl.skipped[(size_t)j]) continue;
            const int64_t orig = pl.order[(size_t)j];
            const int64_t* tri = f + 3 * orig;
            for (int k = 0; k < it[2]; ++k) {
                const int64_t p = pl.plane_list[(size_t)(it[1] + k)];
                const Plane plane = plane_of(origins, normals, p);
                section::Corner c[3];
                for (int a = 0; a < 3; ++a) {
                    const double* x = v + 3 * tri[a];
                    c[a] = section::Corner{x[0], x[1], x[2], section::height(plane, x[0], x[1], x[2]), (int32_t)tri[a]};
                }
                if (!section::crossed(c[0].h, c[1].h, c[2].h)) continue;
                Segment s;
                section::cut_face(c[0], c[1], c[2], (unsigned long long)p << 32 | (unsigned long long)orig, s);
                out.push_back(s);
            }
        }
    }
}

// ---- rules 5 to 7 ---------------------------------------------------------------------------------------------------

struct SectionOut {
    int64_t* contour_off; double* points; int64_t* point_edge; int64_t* point_face; int64_t* contour_plane;
    int8_t* contour_kind; double *contour_area, *contour_length, *contour_centroid; int64_t *plane_off, *selected;
    int64_t n_contours = 0, n_points = 0, n_closed = 0, n_open = 0, n_branched = 0;
};

double dist3(const double* a, const double* b)
{
    const double ex = b[0] - a[0], ey = b[1] - a[1], ez = b[2] - a[2];
    return std::sqrt((ex * ex + ey * ey) + ez * ez);
}

// length-weighted mean of the points of a polyline of m points (closed: its last segment returns to the first point)
void curve_mean(const double* p, int64_t m, bool closed, double* length, double* mean)
{
    double L = 0.0, M[3] = {0.0, 0.0, 0.0};
    const int64_t n_seg = closed ? m : m - 1;
    for (int64_t i = 0; i < n_seg; ++i) {
        const double *a = p + 3 * i, *b = p + 3 * ((i + 1) % m);
        const double len = dist3(a, b);
        L += len;
        for (int k = 0; k < 3; ++k) M[k] += len * (0.5 * (a[k] + b[k]));
    }
    *length = L;
    for (int k = 0; k < 3; ++k) mean[k] = L == 0.0 ? p[k] : M[k] / L;
}

// rule 6 on a closed loop in its listed order, about its own first point: s = the vector area dotted with n; B = the
// sum of the magnitudes of every product that enters W, the scale of W's rounding error
double loop_signed(const double* p, int64_t m, const Plane& pl, double* W_out, double* B_out, double* G)
{
    double A[3] = {0.0, 0.0, 0.0}, W = 0.0, B = 0.0;
    const double an[3] = {std::fabs(pl.nx), std::fabs(pl.ny), std::fabs(pl.nz)};
    G[0] = G[1] = G[2] = 0.0;
    for (int64_t i = 0; i < m; ++i) {
        const double *a = p + 3 * i, *b = p + 3 * ((i + 1) % m);
        const double d[3] = {a[0] - p[0], a[1] - p[1], a[2] - p[2]}, e[3] = {b[0] - p[0], b[1] - p[1], b[2] - p[2]};
        const double c[3] = {d[1] * e[2] - d[2] * e[1], d[2] * e[0] - d[0] * e[2], d[0] * e[1] - d[1] * e[0]};
        for (int k = 0; k < 3; ++k) A[k] += c[k];
        const double w = (c[0] * pl.nx + c[1] * pl.ny) + c[2] * pl.nz;
        W += w;
        const double q[3] = {std::fabs(d[1] * e[2]) + std::fabs(d[2] * e[1]), std::fabs(d[2] * e[0]) + std::fabs(d[0] * e[2]),
                             std::fabs(d[0] * e[1]) + std::fabs(d[1] * e[0])};
        B += (q[0] * an[0] + q[1] * an[1]) + q[2] * an[2];
        for (int k = 0; k < 3; ++k) G[k] += w * (d[k] + e[k]);
    }
    *W_out = W;
    *B_out = B;
    return (A[0] * pl.nx + A[1] * pl.ny) + A[2] * pl.nz;
}

// rule 7: is the origin inside the loop, even-odd, in the projection that drops the axis of the largest |n| component
bool origin_inside(const double* p, int64_t m, const Plane& pl)
{
    const double an[3] = {std::fabs(pl.nx), std::fabs(pl.ny), std::fabs(pl.nz)};
    int drop = 0;
    for (int a = 1; a < 3; ++a) if (an[a] > an[drop]) drop = a;
    const int iu = drop == 0 ? 1 : 0, iv = drop == 2 ? 1 : 2;
    const double o[3] = {pl.ox, pl.oy, pl.oz};
    bool inside = false;
    for (int64_t i = 0; i < m; ++i) {
        const double *a = p + 3 * i, *b = p + 3 * ((i + 1) % m);
        if ((a[iv] > o[iv]) == (b[iv] > o[iv])) continue;
        const double t = ((o[iv] - a[iv]) * (b[iu] - a[iu])) / (b[iv] - a[iv]);
        if (o[iu] < a[iu] + t) inside = !inside;
    }
    return inside;
}

struct KeyEntry { unsigned long long key; int32_t seg, end; };

// The segments of one plane (sorted by face) into its contours, appended to out.
void chain_plane(const Segment* seg, int64_t m, const Plane& pl, int64_t plane, SectionOut& out)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    std::vector<KeyEntry> ent((size_t)(2 * m));
    for (int64_t s = 0; s < m; ++s)
        for (int e = 0; e < 2; ++e)
            ent[(size_t)(2 * s + e)] = KeyEntry{(unsigned long long)(uint32_t)seg[s].e[2 * e] << 32 | (uint32_t)seg[s].e[2 * e + 1], (int32_t)s, e};
    std::sort(ent.begin(), ent.end(), [](const KeyEntry& a, const KeyEntry& b) { return a.key != b.key ? a.key < b.key : a.seg < b.seg; });
    // distinct keys, ascending: key k = entries first[k] .. first[k + 1]
    std::vector<int32_t> first, kid((size_t)(2 * m));
    for (int64_t i = 0; i < 2 * m; ++i) {
        if (i == 0 || ent[(size_t)i].key != ent[(size_t)i - 1].key) first.push_back((int32_t)i);
        kid[(size_t)(2 * ent[(size_t)i].seg + ent[(size_t)i].end)] = (int32_t)first.size() - 1;
    }
    const int64_t K = (int64_t)first.size();
    first.push_back((int32_t)(2 * m));
    auto key_point = [&](int32_t k) { const KeyEntry& e = ent[(size_t)first[(size_t)k]]; return seg[e.seg].p + 3 * e.end; };
    auto degree = [&](int32_t k) { return first[(size_t)k + 1] - first[(size_t)k]; };
    // components of keys: the root is the smallest key
    std::vector<int32_t> root((size_t)K);
    for (int64_t k = 0; k < K; ++k) root[(size_t)k] = (int32_t)k;
    auto find = [&](int32_t k) { while (root[(size_t)k] != k) { root[(size_t)k] = root[(size_t)root[(size_t)k]]; k = root[(size_t)k]; } return k; };
    for (int64_t s = 0; s < m; ++s) {
        const int32_t a = find(kid[(size_t)(2 * s)]), b = find(kid[(size_t)(2 * s + 1)]);
        if (a != b) root[(size_t)std::max(a, b)] = std::min(a, b);
    }
    std::vector<std::vector<int32_t>> members((size_t)K);
    for (int64_t k = 0; k < K; ++k) members[(size_t)find((int32_t)k)].push_back((int32_t)k);

    std::vector<int32_t> walk_key, walk_seg;
    std::vector<double> pts;
    const int64_t first_contour = out.n_contours;
    for (int64_t r = 0; r < K; ++r) {
        const std::vector<int32_t>& keys = members[(size_t)r];
        if (keys.empty()) continue;
        int max_deg = 0, ends[2] = {-1, -1}, n_ends = 0;
        for (int32_t k : keys) {
            max_deg = std::max(max_deg, (int)degree(k));
            if (degree(k) == 1) { if (n_ends < 2) ends[n_ends] = k; ++n_ends; }
        }
        const int64_t c = out.n_contours++;
        out.contour_plane[c] = plane;
        double* cen = out.contour_centroid + 3 * c;
        auto emit = [&](int32_t k, int64_t face) {
            const int64_t at = out.n_points++;
            std::memcpy(out.points + 3 * at, key_point(k), 24);
            out.point_edge[2 * at] = (int64_t)(ent[(size_t)first[(size_t)k]].key >> 32);
            out.point_edge[2 * at + 1] = (int64_t)(ent[(size_t)first[(size_t)k]].key & 0xffffffffull);
            out.point_face[at] = face;
        };
        if (max_deg > 2) {                                             // branched: the keys ascending, no order along it
            for (int32_t k : keys) emit(k, -1);
            double L = 0.0;
            for (int64_t s = 0; s < m; ++s)
                if (find(kid[(size_t)(2 * s)]) == (int32_t)r) L += dist3(seg[s].p, seg[s].p + 3);
            out.contour_kind[c] = 2; out.contour_area[c] = nan; out.contour_length[c] = L;
            cen[0] = cen[1] = cen[2] = nan;
            ++out.n_branched;
        } else {
            const bool open = n_ends == 2;
            const int32_t start = open ? ends[0] : keys[0];
            // the segment to leave the start by: an open end has one; a loop leaves towards its smaller neighbouring key,
            // by the smaller face where both segments lead to the same key
            auto other_key = [&](int32_t s, int32_t k) { return kid[(size_t)(2 * s)] == k ? kid[(size_t)(2 * s + 1)] : kid[(size_t)(2 * s)]; };
            int32_t s = ent[(size_t)first[(size_t)start]].seg;
            if (!open) {
                const int32_t s2 = ent[(size_t)first[(size_t)start] + 1].seg;
                if (other_key(s2, start) < other_key(s, start)) s = s2;
            }
            walk_key.clear(); walk_seg.clear();
            int32_t k = start;
            for (;;) {
                walk_key.push_back(k);
                const int32_t next = other_key(s, k);
                if (next == start) { walk_seg.push_back(s); break; }                  // a loop closes
                walk_seg.push_back(s);
                k = next;
                if (degree(k) == 1) { walk_key.push_back(k); break; }                 // the far end of an open polyline
                const int32_t e0 = ent[(size_t)first[(size_t)k]].seg, e1 = ent[(size_t)first[(size_t)k] + 1].seg;
                s = e0 == s ? e1 : e0;
            }
            const int64_t n = (int64_t)walk_key.size();
            pts.resize((size_t)(3 * n));
            for (int64_t i = 0; i < n; ++i) std::memcpy(pts.data() + 3 * i, key_point(walk_key[(size_t)i]), 24);
            if (open) {
                for (int64_t i = 0; i < n; ++i) emit(walk_key[(size_t)i], i + 1 < n ? (int64_t)(seg[walk_seg[(size_t)i]].key & 0xffffffffull) : -1);
                out.contour_kind[c] = 1; out.contour_area[c] = nan;
                curve_mean(pts.data(), n, false, out.contour_length + c, cen);
                ++out.n_open;
            } else {
                double W, B, G[3];
                double sgn = loop_signed(pts.data(), n, pl, &W, &B, G);
                if (sgn < 0.0) {                                       // the other direction: p0, p(n-1), ..., p1
                    std::reverse(walk_key.begin() + 1, walk_key.end());
                    std::reverse(walk_seg.begin(), walk_seg.end());
                    for (int64_t i = 0; i < n; ++i) std::memcpy(pts.data() + 3 * i, key_point(walk_key[(size_t)i]), 24);
                    sgn = loop_signed(pts.data(), n, pl, &W, &B, G);
                }
                for (int64_t i = 0; i < n; ++i) emit(walk_key[(size_t)i], (int64_t)(seg[walk_seg[(size_t)i]].key & 0xffffffffull));
                out.contour_kind[c] = 0;
                out.contour_area[c] = (0.5 * sgn) / std::sqrt((pl.nx * pl.nx + pl.ny * pl.ny) + pl.nz * pl.nz);
                double mean[3];
                curve_mean(pts.data(), n, true, out.contour_length + c, mean);
                // flat: |W| within twice the rounding bound of its own sum
                const bool flat = !(std::fabs(W) > ((double)(n + 6) * std::numeric_limits<double>::epsilon()) * B);
                for (int a = 0; a < 3; ++a) cen[a] = flat ? mean[a] : pts[(size_t)a] + G[a] / (3.0 * W);
                ++out.n_closed;
            }
        }
        out.contour_off[c + 1] = out.n_points;
    }
    // rule 7
    int64_t best = -1;
    for (int64_t c = first_contour; c < out.n_contours; ++c) {
        if (out.contour_kind[c] != 0) continue;
        const int64_t a = out.contour_off[c], n = out.contour_off[c + 1] - a;
        if (!origin_inside(out.points + 3 * a, n, pl)) continue;
        if (best < 0 || out.contour_area[c] < out.contour_area[best]) best = c;
    }
    out.selected[plane] = best;
}

// sorted segments (by plane, then face) into every output; the arrays hold n_segments contours and 2 n_segments points
void chain_all(const Segment* seg, int64_t n_seg, const double* origins, const double* normals, int64_t n_planes, SectionOut& out)
{
    TraceTimer tt("section: chain and measure");
    out.contour_off[0] = 0;
    int64_t s = 0;
    for (int64_t p = 0; p < n_planes; ++p) {
        out.plane_off[p] = out.n_contours;
        int64_t e = s;
        while (e < n_seg && (int64_t)(seg[e].key >> 32) == p) ++e;
        if (e > s) chain_plane(seg + s, e - s, plane_of(origins, normals, p), p, out);
        else out.selected[p] = -1;
        s = e;
    }
    out.plane_off[n_planes] = out.n_contours;
}

bool sorted_segments(const Segment* seg, int64_t n, int64_t n_planes)
{
    for (int64_t i = 0; i < n; ++i) {
        if ((int64_t)(seg[i].key >> 32) >= n_planes) return false;
        if (i > 0 && !(seg[i - 1].key < seg[i].key)) return false;
        for (int e = 0; e < 2; ++e)
            if (seg[i].e[2 * e] < 0 || !(seg[i].e[2 * e] < seg[i].e[2 * e + 1])) return false;
        if (seg[i].e[0] == seg[i].e[2] && seg[i].e[1] == seg[i].e[3]) return false;
    }
    return true;
}

bool outputs_given(const SectionOut& o, int64_t cap, int64_t n_planes)
{
    if (!o.contour_off || !o.plane_off) return false;
    if (n_planes > 0 && !o.selected) return false;
    if (cap > 0 && (!o.points || !o.point_edge || !o.point_face || !o.contour_plane || !o.contour_kind || !o.contour_area ||
                    !o.contour_length || !o.contour_centroid))
        return false;
    return true;
}

}  // namespace

extern "C" {

int mm_section_plan(const double* v, int64_t nv, const int64_t* f, int64_t nf, const double* origins, const double* normals,
                    int64_t n_planes, int32_t* order, int64_t* info, double* chunk_boxes, int32_t* plane_list,
                    int64_t list_cap, int32_t* items, int64_t item_cap)
{
    if (!info || list_cap < 0 || item_cap < 0 || (list_cap > 0 && !plane_list) || (item_cap > 0 && !items) || (nf > 0 && !order))
        return set_error(MM_ERR_INVALID, "mm_section_plan: bad arguments");
    int rc = plan_args(v, nv, f, nf, nullptr, 0, "mm_section_plan");
    if (rc) return rc;
    if ((rc = check_planes(origins, normals, n_planes, "mm_section_plan"))) return rc;
    SectionPlan pl;
    if ((rc = build_section_plan(v, f, nf, origins, normals, n_planes, "mm_section_plan", pl))) return rc;
    if (nf > 0) std::memcpy(order, pl.order.data(), (size_t)nf * 4);
    info[0] = pl.n_pairs; info[1] = pl.pairs_total; info[2] = pl.ch; info[3] = (int64_t)pl.cbox.size();
    info[4] = pl.n_items(); info[5] = pl.run; info[6] = pl.face_tests; info[7] = pl.n_skipped;
    if (chunk_boxes && !pl.cbox.empty()) std::memcpy(chunk_boxes, pl.cbox.data(), pl.cbox.size() * sizeof(Box3));
    if (std::min(list_cap, pl.n_pairs) > 0) std::memcpy(plane_list, pl.plane_list.data(), (size_t)std::min(list_cap, pl.n_pairs) * 4);
    if (std::min(item_cap, pl.n_items()) > 0) std::memcpy(items, pl.items.data(), (size_t)std::min(item_cap, pl.n_items()) * 16);
    return MM_OK;
}

int mm_section_cut_host(const double* v, int64_t nv, const int64_t* f, int64_t nf, const double* origins,
                        const double* normals, int64_t n_planes, int64_t cap, void* segments, int64_t* n_segments)
{
    if (!n_segments || cap < 0 || (cap > 0 && !segments)) return set_error(MM_ERR_INVALID, "mm_section_cut_host: bad arguments");
    int rc = plan_args(v, nv, f, nf, nullptr, 0, "mm_section_cut_host");
    if (rc) return rc;
    if ((rc = check_planes(origins, normals, n_planes, "mm_section_cut_host"))) return rc;
    SectionPlan pl;
    if ((rc = build_section_plan(v, f, nf, origins, normals, n_planes, "mm_section_cut_host", pl))) return rc;
    std::vector<Segment> seg;
    cut_on_host(pl, v, f, nf, origins, normals, seg);
    std::sort(seg.begin(), seg.end(), [](const Segment& a, const Segment& b) { return a.key < b.key; });
    *n_segments = (int64_t)seg.size();
    if (std::min<int64_t>(cap, (int64_t)seg.size()) > 0)
        std::memcpy(segments, seg.data(), (size_t)std::min<int64_t>(cap, (int64_t)seg.size()) * sizeof(Segment));
    return MM_OK;
}

int mm_section_chain(const void* segments, int64_t n_segments, const double* origins, const double* normals,
                     int64_t n_planes, int64_t* contour_off, double* points, int64_t* point_edge, int64_t* point_face,
                     int64_t* contour_plane, int8_t* contour_kind, double* contour_area, double* contour_length,
                     double* contour_centroid, int64_t* plane_off, int64_t* selected, int64_t* counts)
{
    SectionOut out{contour_off, points, point_edge, point_face, contour_plane, contour_kind, contour_area, contour_length,
                   contour_centroid, plane_off, selected};
    if (!counts || n_segments < 0 || n_segments > kMaxIndex || (n_segments > 0 && !segments) || !outputs_given(out, n_segments, n_planes))
        return set_error(MM_ERR_INVALID, "mm_section_chain: bad arguments");
    const int rc = check_planes(origins, normals, n_planes, "mm_section_chain");
    if (rc) return rc;
    const Segment* seg = (const Segment*)segments;
    if (!sorted_segments(seg, n_segments, n_planes))
        return set_error(MM_ERR_INVALID, "mm_section_chain: the segments are not sorted by (plane, face), or a key is out of range");
    chain_all(seg, n_segments, origins, normals, n_planes, out);
    counts[0] = out.n_contours; counts[1] = out.n_points; counts[2] = out.n_closed; counts[3] = out.n_open; counts[4] = out.n_branched;
    return MM_OK;
}

int mm_mesh_sections(mm_engine* h, const double* v, int64_t nv, const int64_t* f, int64_t nf, const double* origins,
                     const double* normals, int64_t n_planes, int64_t max_segments, int64_t* contour_off, double* points,
                     int64_t* point_edge, int64_t* point_face, int64_t* contour_plane, int8_t* contour_kind,
                     double* contour_area, double* contour_length, double* contour_centroid, int64_t* plane_off,
                     int64_t* selected, mm_section_report* report)
{
    Engine* e;
    int rc = engine_of(h, e);
    if (rc) return rc;
    SectionOut out{contour_off, points, point_edge, point_face, contour_plane, contour_kind, contour_area, contour_length,
                   contour_centroid, plane_off, selected};
    if (!report || max_segments < 0 || max_segments > kMaxIndex || !outputs_given(out, max_segments, std::max<int64_t>(n_planes, 0)))
        return set_error(MM_ERR_INVALID, "mm_mesh_sections: bad arguments");
    if ((rc = plan_args(v, nv, f, nf, nullptr, 0, "mm_mesh_sections"))) return rc;
    if ((rc = check_planes(origins, normals, n_planes, "mm_mesh_sections"))) return rc;
    SectionPlan pl;
    if ((rc = build_section_plan(v, f, nf, origins, normals, n_planes, "mm_mesh_sections", pl))) return rc;

    mm_section_report rep;
    std::memset(&rep, 0, sizeof(rep));
    rep.n_planes = n_planes; rep.n_faces = nf; rep.n_skipped_faces = pl.n_skipped;
    rep.items = pl.n_pairs; rep.items_total = pl.pairs_total; rep.face_tests = pl.face_tests;
    const int64_t n_items = pl.n_items();
    const Segment* seg = nullptr;
    int64_t n_seg = 0;
    StagedPass sp;
    if (n_items > 0) {
        const int64_t cap = std::min(max_segments, pl.face_tests);      // no call finds more segments than it tests faces
        const size_t o_tri = sp.in.take((size_t)nf * 96), o_planes = sp.in.take((size_t)n_planes * 48);
        const size_t o_list = sp.in.take((size_t)pl.n_pairs * 4), o_items = sp.in.take((size_t)n_items * 16);
        const size_t o_cnt = sp.out.take(64), o_seg = sp.out.take((size_t)cap * sizeof(Segment));
        if ((rc = sp.reserve(e))) return rc;
        stage_section_records(pl, v, f, nf, sp.host<double>(o_tri));
        for (int64_t p = 0; p < n_planes; ++p) {
            std::memcpy(sp.host<double>(o_planes) + 6 * p, origins + 3 * p, 24);
            std::memcpy(sp.host<double>(o_planes) + 6 * p + 3, normals + 3 * p, 24);
        }
        std::memcpy(sp.host<int32_t>(o_list), pl.plane_list.data(), (size_t)pl.n_pairs * 4);
        std::memcpy(sp.host<int32_t>(o_items), pl.items.data(), (size_t)n_items * 16);
        MM_TRY_HIP(hipMemcpyAsync(sp.d, sp.h, sp.in.size(), hipMemcpyHostToDevice, e->stream));
        if ((rc = e->profile_begin(e->stream))) return rc;
        const hipError_t he = launch_section_cut(sp.dev_in<int32_t>(o_items), (int)n_items, sp.dev_in<int32_t>(o_list),
                                                 sp.dev_in<double>(o_planes), sp.dev_in<double>(o_tri), (int)nf,
                                                 sp.dev_out<unsigned long long>(o_cnt), sp.dev_out<void>(o_seg),
                                                 (unsigned long long)cap, e->stream);
        if (he != hipSuccess) return hip_error(he, "launch_section_cut");
        if ((rc = e->profile_end(e->stream, (double)pl.face_tests, 0))) return rc;
        MM_TRY_HIP(hipMemcpyAsync(sp.host<unsigned char>(o_cnt), sp.dev_out<unsigned char>(o_cnt), 64, hipMemcpyDeviceToHost, e->stream));
        MM_TRY_HIP(hipStreamSynchronize(e->stream));
        n_seg = (int64_t)sp.host<unsigned long long>(o_cnt)[0];
        if (n_seg < 0 || n_seg > pl.face_tests) return set_error(MM_ERR_HIP, "mm_mesh_sections: segment counter out of range");
        rep.n_segments = n_seg;
        rep.n_launches = section_launches();
        rep.bytes_uploaded = (int64_t)sp.in.size();
        rep.bytes_downloaded = 64;
        if (n_seg > max_segments) {
            *report = rep;
            return set_error(MM_ERR_TOO_LARGE, "mm_mesh_sections: more segments than max_segments");
        }
        if (n_seg > 0) {
            MM_TRY_HIP(hipMemcpyAsync(sp.host<unsigned char>(o_seg), sp.dev_out<unsigned char>(o_seg), (size_t)n_seg * sizeof(Segment),
                                      hipMemcpyDeviceToHost, e->stream));
            MM_TRY_HIP(hipStreamSynchronize(e->stream));
            rep.bytes_downloaded += n_seg * (int64_t)sizeof(Segment);
            Segment* got = sp.host<Segment>(o_seg);
            TraceTimer t_sort("section: sort");
            std::sort(got, got + n_seg, [](const Segment& a, const Segment& b) { return a.key < b.key; });
            t_sort.stop();
            if (!sorted_segments(got, n_seg, n_planes)) return set_error(MM_ERR_HIP, "mm_mesh_sections: segment records out of range");
            seg = got;
        }
    }
    chain_all(seg, n_seg, origins, normals, n_planes, out);
    rep.n_contours = out.n_contours; rep.n_closed = out.n_closed; rep.n_open = out.n_open; rep.n_branched = out.n_branched;
    *report = rep;
    return MM_OK;
}

}  // extern "C"
