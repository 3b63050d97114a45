// mm_clip_kernels.hip -- the device pass of "mesh clipping" (include/mm_ccta.h, rules C2, C4, C5, C7), for gfx950.  The
// mesh, one record per cut face (clip::Record of mm_clip_device.h, written by the host from the sections), the new
// vertices and the cuts are uploaded once and stay resident; int32 indices, every one checked against its range on the
// host.  No output depends on the order in which lanes arrive: the union-find's roots may differ between runs, and only
// root equality and the drop marks (plain byte stores of 1) are read; every position comes from a scan; the status and
// the counters take integer atomics.  No float atomics, no inline assembly; built with -ffp-contract=off.
//
//   k_clip_init      link[x] = x << 1 (a root), frec = -1, the marks, the counters and the statuses zero.
//   k_clip_scatter   frec[face of record r] = r: one record a face (the host found no OVERLAP).
//   k_clip_sides     one lane per vertex: vdrop = it lies on the drop side of some PLANE cut (rule 1).
//   k_clip_union     one lane per face: uf_union of mm_mesh_device.h, parities unused; a face without a record unites
//                    its three vertices, a cut face the two that are not its apex.  launch_weld_jump flattens the links.
//   k_clip_verdict   one lane per record of a LOOP cut, links flat: the roots of the apex and of its neighbour; equal ->
//                    atomicOr of NOT_SEPARATING into the cut's status, else mark[drop-side root] = 1.
//   k_clip_orphan    one lane per record, after a verdict that left every status zero (the marks are complete): a
//                    kept-side vertex of the face is dropped (mark[root] | vdrop) -> atomicOr of KEPT_SIDE_DROPPED.
//   k_clip_keep      vkeep = not (mark[root] or vdrop); launch_trim_scan numbers the kept vertices.
//   k_clip_count     one lane per face: the pieces it leaves (0 to 3), the dropped and the untouched faces counted per
//                    wave (wave_count); k_clip_tile_sum / k_clip_tile_scan / k_clip_offsets scan the counts (the
//                    three-pass scan of mm_trim_kernels.hip over small integers in the place of flags).
//   k_clip_vertices  the kept vertices to their slots, the new ones behind them, vertex_origin.
//   k_clip_emit      one lane per face: corners remapped, the diagonal test on the stored coordinates (clip::face_pieces),
//                    face_origin, face_kind, the null pieces counted per wave.
//   k_clip_rim       one lane per (record on a closed loop, layer): its two extension faces, and its cap face.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mm_device.h"
#include "mm_mesh_device.h"
#include "mm_clip_device.h"
#include "mm_section_device.h"

namespace mm {

using clip::Record;

__global__ void __launch_bounds__(kMeshThreads)
k_clip_init(unsigned int* __restrict__ link, uint8_t* __restrict__ mark, uint8_t* __restrict__ vdrop, long long nv,
            int32_t* __restrict__ frec, long long nf, unsigned long long* __restrict__ counts, int32_t* __restrict__ status,
            long long n_cuts)
{
    const long long n = nv > nf ? nv : nf;
    for (long long i = mesh_tid(); i < n; i += mesh_stride()) {
        if (i < nv) { link[i] = (unsigned int)i << 1; mark[i] = 0; vdrop[i] = 0; }
        if (i < nf) frec[i] = -1;
    }
    for (long long i = mesh_tid(); i < n_cuts; i += mesh_stride()) status[i] = 0;
    if (mesh_tid() < clip_num_counts) counts[mesh_tid()] = 0ull;
}

__global__ void __launch_bounds__(kMeshThreads)
k_clip_scatter(const Record* __restrict__ rec, long long nr, int32_t* __restrict__ frec)
{
    for (long long r = mesh_tid(); r < nr; r += mesh_stride()) frec[rec[r].face] = (int32_t)r;
}

__global__ void __launch_bounds__(kMeshThreads)
k_clip_sides(const double* __restrict__ v, long long nv, const ClipCut* __restrict__ cuts, int n_cuts, uint8_t* __restrict__ vdrop)
{
    for (long long i = mesh_tid(); i < nv; i += mesh_stride()) {
        const double x = v[3 * i], y = v[3 * i + 1], z = v[3 * i + 2];
        uint8_t drop = 0;
        for (int k = 0; k < n_cuts; ++k) {
            const ClipCut c = cuts[k];
            if (c.scope != kClipScopePlane) continue;
            const section::Plane pl{c.o[0], c.o[1], c.o[2], c.n[0], c.n[1], c.n[2]};
            if (section::side(section::height(pl, x, y, z)) != c.keep) drop = 1;
        }
        vdrop[i] = drop;
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_clip_union(const int32_t* __restrict__ face, long long nf, const int32_t* __restrict__ frec, const Record* __restrict__ rec,
             unsigned int* __restrict__ link)
{
    for (long long f = mesh_tid(); f < nf; f += mesh_stride()) {
        const int32_t c0 = face[3 * f], c1 = face[3 * f + 1], c2 = face[3 * f + 2];
        const int32_t r = frec[f];
        if (r < 0) {
            if (c0 != c1) uf_union(link, (unsigned int)c0, (unsigned int)c1, 0u);
            if (c1 != c2) uf_union(link, (unsigned int)c1, (unsigned int)c2, 0u);
        } else {
            const int apex = rec[r].flags & clip::kApexMask;
            const int32_t b = apex == 0 ? c1 : (apex == 1 ? c2 : c0), c = apex == 0 ? c2 : (apex == 1 ? c0 : c1);
            uf_union(link, (unsigned int)b, (unsigned int)c, 0u);
        }
    }
}

// links flat: link[x] >> 1 is the root of x
__global__ void __launch_bounds__(kMeshThreads)
k_clip_verdict(const int32_t* __restrict__ face, const Record* __restrict__ rec, long long nr, const unsigned int* __restrict__ link,
               uint8_t* __restrict__ mark, int32_t* __restrict__ status)
{
    for (long long r = mesh_tid(); r < nr; r += mesh_stride()) {
        const Record q = rec[r];
        if (!(q.flags & clip::kLoopCut)) continue;
        const int apex = q.flags & clip::kApexMask;
        const int32_t a = face[3 * (long long)q.face + apex], b = face[3 * (long long)q.face + (apex == 2 ? 0 : apex + 1)];
        const unsigned int ra = link[a] >> 1, rb = link[b] >> 1;
        if (ra == rb) atomicOr(&status[q.cut], kClipNotSeparating);
        else mark[(q.flags & clip::kApexKept) ? rb : ra] = 1;
    }
}

// links flat, marks complete: every status is zero when this runs, so the only value it leaves is kClipKeptSideDropped
__global__ void __launch_bounds__(kMeshThreads)
k_clip_orphan(const int32_t* __restrict__ face, const Record* __restrict__ rec, long long nr, const unsigned int* __restrict__ link,
              const uint8_t* __restrict__ mark, const uint8_t* __restrict__ vdrop, int32_t* __restrict__ status)
{
    for (long long r = mesh_tid(); r < nr; r += mesh_stride()) {
        const Record q = rec[r];
        const int32_t c0 = face[3 * (long long)q.face], c1 = face[3 * (long long)q.face + 1], c2 = face[3 * (long long)q.face + 2];
        auto dropped = [&](int32_t x) { return (mark[link[x] >> 1] | vdrop[x]) != 0; };
        if (clip::kept_side_dropped(q.flags, dropped(c0), dropped(c1), dropped(c2))) atomicOr(&status[q.cut], kClipKeptSideDropped);
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_clip_keep(const unsigned int* __restrict__ link, const uint8_t* __restrict__ mark, const uint8_t* __restrict__ vdrop, long long nv,
            uint8_t* __restrict__ vkeep)
{
    for (long long i = mesh_tid(); i < nv; i += mesh_stride()) vkeep[i] = (mark[link[i] >> 1] | vdrop[i]) ? 0 : 1;
}

// what the count and the emit kernels share: the pieces of face f with record q, every corner named in the result
static __device__ __forceinline__ clip::Pieces clip_face(const double* __restrict__ v, const double* __restrict__ newv,
                                                         const int32_t* __restrict__ vidx, long long kv, int32_t c0, int32_t c1,
                                                         int32_t c2, const Record& q)
{
    auto old_corner = [&](int32_t i) {
        const int32_t k = vidx[i];
        return clip::Corner{k, clip::Point{v[3 * (long long)i], v[3 * (long long)i + 1], v[3 * (long long)i + 2]}, k < 0};
    };
    auto new_corner = [&](int32_t j) {
        return clip::Corner{(int32_t)(kv + j), clip::Point{newv[3 * (long long)j], newv[3 * (long long)j + 1], newv[3 * (long long)j + 2]}, false};
    };
    return clip::face_pieces(old_corner(c0), old_corner(c1), old_corner(c2), q.flags & clip::kApexMask, new_corner(q.m_ab),
                             new_corner(q.m_ca));
}

// nf_padded: every wave runs the loop whole (the ballots).  vidx: < 0 at a dropped vertex.
__global__ void __launch_bounds__(kMeshThreads)
k_clip_count(const double* __restrict__ v, const double* __restrict__ newv, const int32_t* __restrict__ face, long long nf_padded,
             long long nf, const int32_t* __restrict__ frec, const Record* __restrict__ rec, const int32_t* __restrict__ vidx,
             uint8_t* __restrict__ fcnt, unsigned long long* __restrict__ counts)
{
    for (long long f = mesh_tid(); f < nf_padded; f += mesh_stride()) {
        int n = 0;
        bool untouched = false;
        if (f < nf) {
            const int32_t c0 = face[3 * f], c1 = face[3 * f + 1], c2 = face[3 * f + 2];
            const int32_t r = frec[f];
            if (r < 0) {
                n = (vidx[c0] >= 0 && vidx[c1] >= 0 && vidx[c2] >= 0) ? 1 : 0;
                untouched = n == 1;
            } else {
                const clip::Pieces p = clip_face(v, newv, vidx, 0, c0, c1, c2, rec[r]);
                n = (int)p.apex.kept + (int)p.first.kept + (int)p.second.kept;
            }
            fcnt[f] = (uint8_t)n;
        }
        wave_count(f < nf && n == 0, counts + clip_num_dropped_faces);
        wave_count(untouched, counts + clip_num_untouched);
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_clip_tile_sum(const uint8_t* __restrict__ cnt, long long n, long long* __restrict__ tile_sum)
{
    const long long i0 = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
    long long c = 0;
    for (int j = 0; j < kScanItems; ++j)
        if (i0 + j < n) c += cnt[i0 + j];
    long long total;
    block_exclusive<kMeshThreads>(c, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kMeshThreads)
k_clip_tile_scan(long long* __restrict__ tile_sum, long long n_tiles)
{
    const long long total = scan_tile_sums(tile_sum, n_tiles);
    if (threadIdx.x == 0) tile_sum[n_tiles] = total;
}

// off[i] = the sum of the counts before i
__global__ void __launch_bounds__(kMeshThreads)
k_clip_offsets(const uint8_t* __restrict__ cnt, long long n, const long long* __restrict__ tile_off, int32_t* __restrict__ off)
{
    const long long i0 = (long long)blockIdx.x * kScanTile + (long long)threadIdx.x * kScanItems;
    long long c = 0;
    for (int j = 0; j < kScanItems; ++j)
        if (i0 + j < n) c += cnt[i0 + j];
    long long total;
    long long at = tile_off[blockIdx.x] + block_exclusive<kMeshThreads>(c, &total);
    for (int j = 0; j < kScanItems; ++j) {
        if (i0 + j >= n) break;
        off[i0 + j] = (int32_t)at;
        at += cnt[i0 + j];
    }
}

__global__ void __launch_bounds__(kMeshThreads)
k_clip_vertices(const double* __restrict__ v, long long nv, const int32_t* __restrict__ vidx, const double* __restrict__ newv,
                const int32_t* __restrict__ new_cut, long long n_new, long long kv, double* __restrict__ out_v,
                int32_t* __restrict__ vorigin)
{
    for (long long i = mesh_tid(); i < nv + n_new; i += mesh_stride()) {
        const bool old = i < nv;
        const long long j = i - nv;
        const long long k = old ? (long long)vidx[i] : kv + j;
        if (k < 0) continue;
        const double* src = old ? v + 3 * i : newv + 3 * j;
        out_v[3 * k] = src[0];
        out_v[3 * k + 1] = src[1];
        out_v[3 * k + 2] = src[2];
        vorigin[k] = old ? (int32_t)i : -1 - new_cut[j];
    }
}

static __device__ __forceinline__ void clip_store(int32_t* __restrict__ out_f, int32_t* __restrict__ forigin, uint8_t* __restrict__ fkind,
                                                  long long at, int32_t i0, int32_t i1, int32_t i2, int32_t origin, uint8_t kind)
{
    out_f[3 * at] = i0;
    out_f[3 * at + 1] = i1;
    out_f[3 * at + 2] = i2;
    forigin[at] = origin;
    fkind[at] = kind;
}

__global__ void __launch_bounds__(kMeshThreads)
k_clip_emit(const double* __restrict__ v, const double* __restrict__ newv, const int32_t* __restrict__ face, long long nf_padded,
            long long nf, const int32_t* __restrict__ frec, const Record* __restrict__ rec, const int32_t* __restrict__ vidx,
            long long kv, const uint8_t* __restrict__ fcnt, const int32_t* __restrict__ foff, int32_t* __restrict__ out_f,
            int32_t* __restrict__ forigin, uint8_t* __restrict__ fkind, unsigned long long* __restrict__ counts)
{
    for (long long f = mesh_tid(); f < nf_padded; f += mesh_stride()) {
        int nulls = 0;
        if (f < nf && fcnt[f]) {
            const int32_t c0 = face[3 * f], c1 = face[3 * f + 1], c2 = face[3 * f + 2];
            const int32_t r = frec[f];
            long long at = foff[f];
            if (r < 0) {
                clip_store(out_f, forigin, fkind, at, vidx[c0], vidx[c1], vidx[c2], (int32_t)f, kClipUntouched);
            } else {
                const clip::Pieces p = clip_face(v, newv, vidx, kv, c0, c1, c2, rec[r]);
                if (p.apex.kept) {
                    clip_store(out_f, forigin, fkind, at++, p.apex.i0, p.apex.i1, p.apex.i2, (int32_t)f, kClipPiece);
                    nulls += p.apex.null;
                }
                if (p.first.kept) {
                    clip_store(out_f, forigin, fkind, at++, p.first.i0, p.first.i1, p.first.i2, (int32_t)f, kClipPiece);
                    nulls += p.first.null;
                }
                if (p.second.kept) {
                    clip_store(out_f, forigin, fkind, at++, p.second.i0, p.second.i1, p.second.i2, (int32_t)f, kClipPiece);
                    nulls += p.second.null;
                }
            }
        }
        for (int k = 1; k <= 3; ++k) wave_count(nulls >= k, counts + clip_num_null_pieces);
    }
}

// one lane per (record, layer): layer j < layers gives the two extension faces between rings j and j + 1, layer == layers
// the cap face (with_cap).  first_ext / first_cap: the result's first extension and cap face.  kv + the name of a new
// vertex is its index; ring 0 is the rim itself.
__global__ void __launch_bounds__(kMeshThreads)
k_clip_rim(const Record* __restrict__ rec, long long nr, int layers, int with_cap, long long kv, long long first_ext, long long first_cap,
           int32_t* __restrict__ out_f, int32_t* __restrict__ forigin, uint8_t* __restrict__ fkind)
{
    const long long per = (long long)layers + 1;
    for (long long i = mesh_tid(); i < nr * per; i += mesh_stride()) {
        const Record q = rec[i / per];
        const int j = (int)(i % per);
        if (!(q.flags & clip::kClosedRim)) continue;
        const bool fwd = clip::rim_runs_ab_to_ca(q.flags);
        const int32_t x0 = fwd ? q.m_ab : q.m_ca, y0 = fwd ? q.m_ca : q.m_ab, xr = fwd ? q.r_ab : q.r_ca, yr = fwd ? q.r_ca : q.r_ab;
        auto ring = [&](int32_t rim, int32_t first_ring, int k) {
            return (int32_t)(kv + (k == 0 ? (long long)rim : (long long)first_ring + (long long)(k - 1) * q.ring_stride));
        };
        if (j < layers) {
            const long long at = first_ext + q.ext_at + (long long)j * 2 * q.ring_stride;
            const int32_t xj = ring(x0, xr, j), yj = ring(y0, yr, j), xn = ring(x0, xr, j + 1), yn = ring(y0, yr, j + 1);
            clip_store(out_f, forigin, fkind, at, yj, xj, xn, -1 - q.cut, kClipExtension);
            clip_store(out_f, forigin, fkind, at + 1, yj, xn, yn, -1 - q.cut, kClipExtension);
        } else if (with_cap) {
            clip_store(out_f, forigin, fkind, first_cap + q.cap_at, ring(y0, yr, layers), ring(x0, xr, layers), (int32_t)(kv + q.centre),
                       -1 - q.cut, kClipCap);
        }
    }
}

// ---- launchers: each returns the error of a launch that failed; *launches += the kernels it launched ----

hipError_t launch_clip_unions(const double* v, long long nv, const int32_t* face, long long nf, const void* rec, long long nr,
                              const ClipCut* cuts, int n_cuts, unsigned int* link, uint8_t* mark, uint8_t* vdrop, int32_t* frec,
                              unsigned long long* counts, int32_t* status, int* launches, hipStream_t s)
{
    MESH_LAUNCH(k_clip_init, mesh_grid(nv > nf ? nv : nf), link, mark, vdrop, nv, frec, nf, counts, status, (long long)n_cuts);
    MESH_LAUNCH(k_clip_scatter, mesh_grid(nr), (const Record*)rec, nr, frec);
    MESH_LAUNCH(k_clip_sides, mesh_grid(nv), v, nv, cuts, n_cuts, vdrop);
    MESH_LAUNCH(k_clip_union, mesh_grid(nf), face, nf, frec, (const Record*)rec, link);
    *launches += 4;
    return hipSuccess;
}

hipError_t launch_clip_verdict(const int32_t* face, const void* rec, long long nr, const unsigned int* link, uint8_t* mark,
                               int32_t* status, int* launches, hipStream_t s)
{
    MESH_LAUNCH(k_clip_verdict, mesh_grid(nr), face, (const Record*)rec, nr, link, mark, status);
    *launches += 1;
    return hipSuccess;
}

hipError_t launch_clip_orphan(const int32_t* face, const void* rec, long long nr, const unsigned int* link, const uint8_t* mark,
                              const uint8_t* vdrop, int32_t* status, int* launches, hipStream_t s)
{
    MESH_LAUNCH(k_clip_orphan, mesh_grid(nr), face, (const Record*)rec, nr, link, mark, vdrop, status);
    *launches += 1;
    return hipSuccess;
}

size_t clip_scan_tiles(long long n) { return scan_tiles(n); }

hipError_t launch_clip_counts(const double* v, long long nv, const double* newv, const int32_t* face, long long nf, const int32_t* frec,
                              const void* rec, const unsigned int* link, const uint8_t* mark, const uint8_t* vdrop, uint8_t* vkeep,
                              int32_t* vidx, long long* vtile, uint8_t* fcnt, int32_t* foff, long long* ftile,
                              unsigned long long* counts, int* launches, hipStream_t s)
{
    MESH_LAUNCH(k_clip_keep, mesh_grid(nv), link, mark, vdrop, nv, vkeep);
    const hipError_t he = launch_trim_scan(vkeep, nv, vtile, vidx, s);
    if (he != hipSuccess) return he;
    *launches += 1 + (scan_tiles(nv) ? 3 : 0);
    MESH_LAUNCH(k_clip_count, mesh_grid(nf), v, newv, face, mesh_pad(nf), nf, frec, (const Record*)rec, vidx, fcnt, counts);
    *launches += 1;
    const long long tiles = (long long)scan_tiles(nf);
    if (tiles == 0) return hipMemsetAsync(ftile, 0, 8, s);
    MESH_LAUNCH(k_clip_tile_sum, (unsigned)tiles, fcnt, nf, ftile);
    MESH_LAUNCH(k_clip_tile_scan, 1u, ftile, tiles);
    MESH_LAUNCH(k_clip_offsets, (unsigned)tiles, fcnt, nf, ftile, foff);
    *launches += 3;
    return hipSuccess;
}

hipError_t launch_clip_emit(const double* v, long long nv, const double* newv, const int32_t* new_cut, long long n_new,
                            const int32_t* face, long long nf, const int32_t* frec, const void* rec, long long nr, const int32_t* vidx,
                            long long kv, const uint8_t* fcnt, const int32_t* foff, int layers, int with_cap, long long first_ext,
                            long long first_cap, double* out_v, int32_t* vorigin, int32_t* out_f, int32_t* forigin, uint8_t* fkind,
                            unsigned long long* counts, int* launches, hipStream_t s)
{
    MESH_LAUNCH(k_clip_vertices, mesh_grid(nv + n_new), v, nv, vidx, newv, new_cut, n_new, kv, out_v, vorigin);
    MESH_LAUNCH(k_clip_emit, mesh_grid(nf), v, newv, face, mesh_pad(nf), nf, frec, (const Record*)rec, vidx, kv, fcnt, foff, out_f,
                forigin, fkind, counts);
    MESH_LAUNCH(k_clip_rim, mesh_grid(nr * ((long long)layers + 1)), (const Record*)rec, nr, layers, with_cap, kv, first_ext, first_cap,
                out_f, forigin, fkind);
    *launches += 3;
    return hipSuccess;
}

}  // namespace mm
