// mm_stage.h -- what the CCTA host files (mm_ccta, mm_shape, mm_branch, mm_discretize, mm_bspline, mm_trim, mm_stitch,
// mm_close, mm_rim, mm_smooth, mm_relax, mm_refine, mm_flip, mm_collapse, mm_surface, mm_repair, mm_geodesic, mm_intersect,
// mm_section, mm_clip .cpp) share when they stage points or a mesh on the engine's grow-only buffers: the engine behind the
// handle, 256-byte carving (typed: one statement a buffer), the staged pass of the point kernels, the mesh argument
// check, the face checks and the int64 <-> int32 face copies, the mesh upload, a counter block's read, the edge table's
// layout, a compaction's counts, the winding stage.  The scratch layouts of the mesh passes are in mm_mesh_layout.h.
// Header-only; internal.
#pragma once

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "mm_engine.h"

#define MM_TRY_HIP(call)                                          \
    do {                                                          \
        const hipError_t e__ = (call);                            \
        if (e__ != hipSuccess) return hip_error(e__, #call);      \
    } while (0)

namespace mm {

inline size_t up256(size_t v) { return (v + 255) / 256 * 256; }

constexpr int64_t kMaxIndex = INT32_MAX;   // device indices are int32: nv and nf stay below 2^31

// the engine behind the handle, with its device selected for the calling thread
inline int engine_of(mm_engine* h, Engine*& e)
{
    e = reinterpret_cast<Engine*>(h);
    if (!e) return set_error(MM_ERR_INVALID, "engine == NULL");
    const hipError_t he = hipSetDevice(e->device);
    if (he != hipSuccess) return hip_error(he, "hipSetDevice");
    return MM_OK;
}

// log2 of the smallest table of at least n slots, never fewer than 256
inline int log2_at_least(unsigned long long n)
{
    int l = 8;
    while ((1ull << l) < n) ++l;
    return l;
}

// Consecutive buffers, each starting on a multiple of 256 bytes.  take() reserves bytes and returns their offset.  place()
// reserves count elements of the pointer's type and points p at them, so a buffer's size and its type are one statement:
// a layout is one function over a Carve that runs twice, measuring (base == nullptr: p = nullptr) and then placing.
struct Carve {
    unsigned char* base = nullptr;
    size_t o = 0;
    size_t take(size_t bytes) { const size_t at = o; o = up256(o + bytes); return at; }
    template <class T> size_t place(T*& p, size_t count)
    {
        const size_t at = take(count * sizeof(T));
        p = base ? (T*)(base + at) : nullptr;
        return at;
    }
    size_t size() const { return o; }
};

// lay(Carve&) measured, buf grown to that size, lay placed over it
template <class Lay> int carve_on(Engine* e, Engine::Buf& buf, Lay lay)
{
    Carve measure;
    lay(measure);
    if (const int rc = e->ensure(buf, measure.size(), false)) return rc;
    Carve c{(unsigned char*)buf.p};
    lay(c);
    return MM_OK;
}

// One pass of a point kernel over e->host_pts (pinned) and e->dev_pts: inputs, outputs and device-only scratch, carved
// apart.  On the device they follow each other in that order; on the host the downloaded outputs take the inputs'
// place.  reserve() after the carving, fill host(), run() the launch, read host(): one copy each way, one synchronise.
struct StagedPass {
    Carve in, out, scratch;
    Engine* e = nullptr;
    unsigned char *h = nullptr, *d = nullptr;

    int reserve(Engine* engine)
    {
        e = engine;
        int rc = e->ensure(e->host_pts, std::max(in.size(), out.size()), true);
        if (rc) return rc;
        if ((rc = e->ensure(e->dev_pts, in.size() + out.size() + scratch.size(), false))) return rc;
        h = (unsigned char*)e->host_pts.p;
        d = (unsigned char*)e->dev_pts.p;
        return MM_OK;
    }
    template <class T> T* host(size_t at) const { return (T*)(h + at); }   // an input before run(), an output after
    template <class T> T* dev_in(size_t at) const { return (T*)(d + at); }
    template <class T> T* dev_out(size_t at) const { return (T*)(d + in.size() + at); }
    template <class T> T* dev_scratch(size_t at) const { return (T*)(d + in.size() + out.size() + at); }

    // the inputs up, launch() between the engine's profile marks (evals = the pair evaluations it reports), the outputs
    // down, synchronised
    template <class Launch> int run(double evals, const char* what, Launch launch) const
    {
        MM_TRY_HIP(hipMemcpyAsync(d, h, in.size(), hipMemcpyHostToDevice, e->stream));
        int rc = e->profile_begin(e->stream);
        if (rc) return rc;
        const hipError_t he = launch();
        if (he != hipSuccess) return hip_error(he, what);
        if ((rc = e->profile_end(e->stream, evals, 0))) return rc;
        MM_TRY_HIP(hipMemcpyAsync(h, d + in.size(), out.size(), hipMemcpyDeviceToHost, e->stream));
        MM_TRY_HIP(hipStreamSynchronize(e->stream));
        return MM_OK;
    }
};

// The work items of a pass of n_jobs jobs, each its own points (pt_off) against its own small set (set_off): one per
// block of block_points points, job-major; a job with an empty set gets none.  Returns the pair evaluations.
inline double point_blocks(int n_jobs, const int64_t* pt_off, const int64_t* set_off, int block_points,
                           std::vector<PointWork>& work)
{
    double evals = 0.0;
    for (int j = 0; j < n_jobs; ++j) {
        const int64_t np = pt_off[j + 1] - pt_off[j], ns = set_off[j + 1] - set_off[j];
        if (ns == 0) continue;
        for (int64_t p0 = 0; p0 < np; p0 += block_points) work.push_back(PointWork{j, (int32_t)p0});
        evals += (double)np * (double)ns;
    }
    return evals;
}

// The pass k_slice_nearest and k_cl_morph share: every point of every job (pts: xyz triples) against that job's small
// set of set_doubles doubles an entry, which fill_set writes into the pinned buffer.  idx and xyz, per point at the
// point's position, are written for the jobs whose set is not empty; the caller settles the others.
template <class Job, class FillSet>
int nearest_pass(Engine* e, const std::vector<Job>& jobs, const int64_t* pt_off, const double* pts, const int64_t* set_off,
                 int set_doubles, FillSet fill_set, int block_points,
                 hipError_t (*launch)(const Job*, const PointWork*, int, const double*, const double*, int32_t*, double*,
                                      hipStream_t),
                 const char* what, int32_t* idx, double* xyz)
{
    const int n_jobs = (int)jobs.size();
    const size_t NP = (size_t)pt_off[n_jobs], NS = (size_t)set_off[n_jobs];
    std::vector<PointWork> work;
    const double evals = point_blocks(n_jobs, pt_off, set_off, block_points, work);
    if (work.empty()) return MM_OK;
    StagedPass sp;
    const size_t o_pts = sp.in.take(NP * 24), o_set = sp.in.take(NS * (size_t)set_doubles * 8);
    const size_t o_jobs = sp.in.take(jobs.size() * sizeof(Job)), o_work = sp.in.take(work.size() * sizeof(PointWork));
    const size_t o_idx = sp.out.take(NP * 4), o_xyz = sp.out.take(NP * 24);
    int rc = sp.reserve(e);
    if (rc) return rc;
    std::memcpy(sp.host<double>(o_pts), pts, NP * 24);
    fill_set(sp.host<double>(o_set));
    std::memcpy(sp.host<Job>(o_jobs), jobs.data(), jobs.size() * sizeof(Job));
    std::memcpy(sp.host<PointWork>(o_work), work.data(), work.size() * sizeof(PointWork));
    rc = sp.run(evals, what, [&] {
        return launch(sp.dev_in<Job>(o_jobs), sp.dev_in<PointWork>(o_work), (int)work.size(), sp.dev_in<double>(o_pts),
                      sp.dev_in<double>(o_set), sp.dev_out<int32_t>(o_idx), sp.dev_out<double>(o_xyz), e->stream);
    });
    if (rc) return rc;
    for (int j = 0; j < n_jobs; ++j) {
        if (set_off[j + 1] == set_off[j]) continue;
        const size_t lo = (size_t)pt_off[j], n = (size_t)pt_off[j + 1] - lo;
        std::memcpy(idx + lo, sp.host<int32_t>(o_idx) + lo, n * 4);
        std::memcpy(xyz + 3 * lo, sp.host<double>(o_xyz) + 3 * lo, n * 24);
    }
    return MM_OK;
}

// every one of the 3 nf indices in [0, nv)
inline int faces_in_range(const int64_t* faces, int64_t nf, int64_t nv, const char* who)
{
    for (int64_t k = 0; k < 3 * nf; ++k)
        if (faces[k] < 0 || faces[k] >= nv) return set_error(MM_ERR_INVALID, std::string(who) + ": face index out of range");
    return MM_OK;
}

// The checks every mesh entry point shares: nv and nf in range, the arrays present (the vertices where the call reads
// them), every index in range, and 6 nf, the edge table's insertions doubled, below 2^31.
inline int mesh_args(const char* who, const double* vertices, int64_t nv, const int64_t* faces, int64_t nf, bool need_vertices)
{
    if (nv < 0 || nf < 0 || nv > kMaxIndex || nf > kMaxIndex || (need_vertices && nv > 0 && !vertices) || (nf > 0 && !faces))
        return set_error(MM_ERR_INVALID, std::string(who) + ": bad arguments");
    if (const int rc = faces_in_range(faces, nf, nv, who)) return rc;
    if (6 * nf > kMaxIndex) return set_error(MM_ERR_TOO_LARGE, std::string(who) + ": 6 nf passes 2^31");
    return MM_OK;
}

// checked indices to the device's int32 (base: the part's first vertex) and back
inline void narrow_faces(int32_t* dst, const int64_t* src, int64_t n_indices, int64_t base = 0)
{
    for (int64_t k = 0; k < n_indices; ++k) dst[k] = (int32_t)(src[k] + base);
}

inline void widen_faces(int64_t* dst, const int32_t* src, int64_t n_indices)
{
    for (int64_t k = 0; k < n_indices; ++k) dst[k] = src[k];
}

// [vertices | int32 faces | mask (nullable)] through e->host_pts into e->dev_pts in one copy, queued on the stream.
// host_bytes: what the caller's downloads need of e->host_pts.
struct MeshUp {
    const double* v = nullptr;
    int32_t* face = nullptr;
    const uint8_t* pin = nullptr;          // nullptr without a mask
    size_t up_bytes = 0;
};
inline int mesh_upload(Engine* e, const double* vertices, int64_t nv, const int64_t* faces, int64_t nf, const uint8_t* mask,
                       size_t host_bytes, MeshUp& m)
{
    const size_t vbytes = (size_t)nv * 24, fbytes = (size_t)nf * 12;
    m.up_bytes = vbytes + fbytes + (mask ? (size_t)nv : 0);
    if (const int rc = e->ensure(e->host_pts, std::max(m.up_bytes, host_bytes) + 512, true)) return rc;
    if (const int rc = e->ensure(e->dev_pts, m.up_bytes, false)) return rc;
    unsigned char* hb = (unsigned char*)e->host_pts.p;
    unsigned char* b = (unsigned char*)e->dev_pts.p;
    std::memcpy(hb, vertices, vbytes);
    narrow_faces((int32_t*)(hb + vbytes), faces, 3 * nf);
    if (mask) std::memcpy(hb + vbytes + fbytes, mask, (size_t)nv);
    MM_TRY_HIP(hipMemcpyAsync(b, hb, m.up_bytes, hipMemcpyHostToDevice, e->stream));
    m.v = (const double*)b;
    m.face = (int32_t*)(b + vbytes);
    m.pin = mask ? b + vbytes + fbytes : nullptr;
    return MM_OK;
}

// a pass's counter block through the first words of e->host_pts (behind the upload in stream order); synchronises
inline int read_words(Engine* e, const unsigned long long* dev_counts, size_t n_words, const unsigned long long** words)
{
    MM_TRY_HIP(hipMemcpyAsync(e->host_pts.p, dev_counts, n_words * 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    *words = (const unsigned long long*)e->host_pts.p;
    return MM_OK;
}

// The edge table of launch_weld_edges: 2^log2_e slots, at least 6 nf (twice the 3 nf insertions of a pass), in three
// planes back to back -- keys (8 bytes a slot), counts (4), the two owners (8).
struct EdgeTable {
    unsigned long long* keys = nullptr;
    unsigned int *cnt = nullptr, *own = nullptr;
    int log2_e = 8;

    static int log2_slots(int64_t nf) { return log2_at_least(6ull * (unsigned long long)nf); }
    size_t slots() const { return (size_t)1 << log2_e; }
    void lay(Carve& c, int64_t nf)
    {
        log2_e = log2_slots(nf);
        c.place(keys, slots()); c.place(cnt, slots()); c.place(own, 2 * slots());
    }
};

// The sorted vertex adjacency of mm_smooth_kernels.hip (mm_smooth.cpp and mm_relax.cpp build it): its device buffers,
// laid out behind whatever the caller placed first.  nb takes the place of the edge table's owner words (8 bytes a slot,
// at least 6 nf slots): the fill runs behind the insertion, which alone writes them.  The caller points counts at four
// words of its own.
struct CsrDev {
    EdgeTable edges;
    int32_t *deg = nullptr, *off = nullptr, *nb = nullptr;
    long long* tile = nullptr;
    unsigned long long* counts = nullptr;  // [0] edges, [1] isolated vertices, [2] the longest row, [3] spare

    void lay(Carve& c, int64_t nf, int64_t nv)
    {
        edges.lay(c, nf);
        c.place(deg, (size_t)nv); c.place(off, (size_t)nv + 1); c.place(tile, mesh_csr_tiles(nv) + 1);
        nb = (int32_t*)edges.own;
    }
};

inline int csr_build(Engine* e, const CsrDev& d, const int32_t* face, int64_t nf, int64_t nv, int* launches)
{
    const EdgeTable& t = d.edges;
    MM_TRY_HIP(launch_weld_edges(face, nf, t.keys, t.cnt, t.own, t.log2_e, e->stream));
    ++*launches;                                                       // nf > 0: the insertion ran
    MM_TRY_HIP(launch_mesh_csr(t.keys, t.log2_e, nv, d.deg, d.off, d.tile, d.nb, d.counts, launches, e->stream));
    return MM_OK;
}

// The counts a compaction kept: the last entry of each launch_trim_scan tile array (vertices, then faces), through the
// first 16 bytes of e->host_pts.  Synchronises the stream.
inline int scan_totals(Engine* e, const long long* vtile, int64_t nv, const long long* ftile, int64_t nf, long long* kv,
                       long long* kf, const char* who)
{
    long long* ht = (long long*)e->host_pts.p;
    MM_TRY_HIP(hipMemcpyAsync(ht, vtile + trim_scan_tiles(nv), 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipMemcpyAsync(ht + 1, ftile + trim_scan_tiles(nf), 8, hipMemcpyDeviceToHost, e->stream));
    MM_TRY_HIP(hipStreamSynchronize(e->stream));
    *kv = ht[0]; *kf = ht[1];
    if (*kv < 0 || *kv > nv || *kf < 0 || *kf > nf)
        return set_error(MM_ERR_HIP, std::string(who) + ": compaction count out of range");
    return MM_OK;
}

// The winding stage of the mesh assembly (mm_stitch.cpp; mm_close.cpp runs it too), on nf int32 faces on the device, in
// place: the edge table (keys, cnt, own: 2^log2_e slots, at least 6 nf), with `fix` the parity union-find (link: nf
// words; changed: one) and the flips (*n_flipped += their number), then the edge report (edge_counts[0..2] += open,
// non-manifold, conflicting edges).  The table and link stay as built: own's directions are those before the flips.
// The first word of e->host_pts takes the round flags.  *rounds = the union-find's launches.
struct WindDev {
    unsigned long long* keys; unsigned int *cnt, *own, *link, *changed;
    unsigned long long *n_flipped, *edge_counts;
    int log2_e;
};
int weld_wind(Engine* e, const WindDev& d, int32_t* face, int64_t nf, bool fix, int64_t* rounds);

}  // namespace mm
