// mm_mesh_stage.h -- what the CCTA host files (mm_ccta, mm_shape, mm_branch, mm_discretize, mm_trim, mm_stitch,
// mm_close, mm_rim, mm_smooth .cpp) share when they stage a mesh on the engine's grow-only buffers: the engine behind
// the handle, 256-byte carving, the face checks and the int64 <-> int32 face copies, the edge table's layout, the
// read-back of a compaction's counts, and the winding stage two of them run.  Header-only; internal.
#pragma once

#include <climits>
#include <cstdint>
#include <string>

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

// Offsets of consecutive buffers, each starting on a multiple of 256 bytes.
struct Carve {
    size_t o = 0;
    size_t take(size_t bytes) { const size_t at = o; o = up256(o + bytes); return at; }
    size_t size() const { return o; }
};

// every one of the 3 nf indices in [0, nv)
inline int faces_in_range(const int64_t* faces, int64_t nf, int64_t nv, const char* who)
{
    for (int64_t k = 0; k < 3 * nf; ++k)
        if (faces[k] < 0 || faces[k] >= nv) return set_error(MM_ERR_INVALID, std::string(who) + ": face index out of range");
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

// The edge table of launch_weld_edges: 2^log2_e slots, at least 6 nf (twice the 3 nf insertions of a pass), in three
// planes -- keys (8 bytes a slot), counts (4), the two owners (8).  plan() carves them back to back, bind() places them.
struct EdgeTable {
    size_t o_keys = 0, o_cnt = 0, o_own = 0;
    unsigned long long* keys = nullptr;
    unsigned int *cnt = nullptr, *own = nullptr;
    int log2_e = 8;

    static int log2_slots(int64_t nf) { return log2_at_least(6ull * (unsigned long long)nf); }
    void plan(Carve& c, int64_t nf)
    {
        log2_e = log2_slots(nf);
        const size_t cap = (size_t)1 << log2_e;
        o_keys = c.take(cap * 8); o_cnt = c.take(cap * 4); o_own = c.take(cap * 8);
    }
    void bind(unsigned char* b)
    {
        keys = (unsigned long long*)(b + o_keys); cnt = (unsigned int*)(b + o_cnt); own = (unsigned int*)(b + o_own);
    }
};

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
