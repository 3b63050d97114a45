// mm_mesh_layout.h -- the scratch layouts of the mesh passes that carve e->dev_raw (mm_refine, mm_flip, mm_collapse,
// mm_repair, mm_geodesic .cpp): a struct of typed device pointers and one lay() each, which states every buffer once --
// its place in the sequence, its element count, and through the pointer its element size.  carve_on (mm_stage.h) runs
// lay() twice, measuring and placing.  DESIGN 4.23 rests on these sequences: which buffer follows which decides what
// stale bytes a pass can meet, and tests/stage_host.cpp holds their sizes and offsets to recorded values.
// Host only; internal.
#pragma once

#include "mm_stage.h"

namespace mm {

// what a refine pass over nf faces needs beside the mesh; list: the edge list of mm_mesh_edge_lengths
constexpr size_t kRefineWords = 16;                                    // the counters of mm_refine_kernels.hip, then the volume
struct RefineScratch {
    EdgeTable t;
    unsigned int* slot; uint8_t* code; int32_t* foff; long long* tile; unsigned long long* counts;
    double *sa, *sb; unsigned char* list;

    void lay(Carve& c, int64_t nf, size_t list_bytes = 0)
    {
        const size_t Fn = (size_t)nf;
        t.lay(c, nf);
        c.place(slot, 3 * Fn); c.place(code, Fn); c.place(foff, Fn);
        c.place(tile, refine_tiles(nf) + 1); c.place(counts, kRefineWords);
        c.place(sa, Fn); c.place(sb, weld_sum_scratch(nf));
        c.place(list, list_bytes);
    }
};

// a flip pass: the edge table with the first corners, the priorities, the opposite corners, the vertex words, best, the
// counters, the volume's scratch
struct FlipScratch {
    EdgeTable t;
    unsigned int *first, *vw;
    unsigned long long *prio, *best, *counts;
    int32_t* opp;
    double *sa, *sb;

    void lay(Carve& c, int64_t nv, int64_t nf)
    {
        t.lay(c, nf);
        const size_t cap = t.slots(), V = (size_t)nv, Fn = (size_t)nf;
        c.place(first, cap); c.place(prio, cap); c.place(opp, 2 * cap);
        c.place(vw, V); c.place(best, V); c.place(counts, flip_num_words);
        c.place(sa, Fn); c.place(sb, weld_sum_scratch(nf));
    }
};

// a collapse pass: the flip's planes with the two ends (rk) for the opposite corners, the adjacency rows apart from the
// table's owner words (the collapse reads both), the liveness bytes, the links r -> k; then what the end needs: the
// scans, the compacted mesh, origin and target, the volume's scratch
struct CollapseScratch {
    EdgeTable t;
    unsigned int *first, *vw;
    unsigned long long *prio, *best, *counts, *csr_counts;
    int32_t *rk, *deg, *off, *nb, *to, *vidx, *fidx, *out_f, *origin, *target;
    uint8_t *fkeep, *vkeep;
    long long *tile, *vtile, *ftile;
    double *out_v, *sa, *sb;

    void lay(Carve& c, int64_t nv, int64_t nf)
    {
        t.lay(c, nf);
        const size_t cap = t.slots(), V = (size_t)nv, Fn = (size_t)nf;
        c.place(first, cap); c.place(prio, cap); c.place(rk, 2 * cap);
        c.place(vw, V); c.place(best, V); c.place(counts, col_num_words);
        c.place(csr_counts, 4);
        c.place(deg, V); c.place(off, V + 1); c.place(tile, mesh_csr_tiles(nv) + 1);
        c.place(nb, cap);                                              // twice the edges: at most 6 nf <= cap entries
        c.place(fkeep, Fn); c.place(vkeep, V); c.place(to, V);
        c.place(vtile, trim_scan_tiles(nv) + 1); c.place(ftile, trim_scan_tiles(nf) + 1);
        c.place(vidx, V); c.place(fidx, Fn);
        c.place(out_v, 3 * V); c.place(out_f, 3 * Fn); c.place(origin, V); c.place(target, V);
        c.place(sa, Fn); c.place(sb, weld_sum_scratch(nf));
    }
};

// the repair: the names (rep), the faces through them (wf), q, the face slots, the liveness bytes, one int32 table for
// vertices and then faces, the edge table's corner slots and the four planes of the two largest keys, the corner links,
// the planes of the split, the three scans, the counters, and the output: the vertices kept and the new ones (at most
// one a corner), faces, origin, target
struct RepairScratch {
    EdgeTable t;
    int log2_v, log2_f;
    int32_t *rep, *wf, *frep, *table, *m1f, *m2f, *vidx, *fidx, *cidx, *out_f, *origin, *target;
    unsigned long long *qb, *m1q, *m2q, *counts;
    unsigned int *eslot, *link, *changed, *vmin, *wmin, *wmax;
    uint8_t *fkeep, *ref, *vsplit, *vkeep, *isnew, *vback, *mixed, *cback;
    long long *vtile, *ftile, *ctile;
    double* out_v;

    void lay(Carve& c, int64_t nv, int64_t nf)
    {
        t.lay(c, nf);
        const size_t cap = t.slots(), V = (size_t)nv, Fn = (size_t)nf, Cn = 3 * Fn;
        log2_v = log2_at_least(2ull * V); log2_f = log2_at_least(2ull * Fn);
        c.place(rep, V); c.place(wf, Cn); c.place(qb, Fn); c.place(frep, Fn);
        c.place(fkeep, Fn); c.place(table, (size_t)1 << std::max(log2_v, log2_f));
        c.place(eslot, Cn); c.place(m1q, cap); c.place(m2q, cap); c.place(m1f, cap);
        c.place(m2f, cap); c.place(link, Cn); c.place(changed, 1);
        c.place(vmin, V); c.place(ref, V); c.place(vsplit, V); c.place(vkeep, V); c.place(isnew, Cn);
        c.place(wmin, V); c.place(wmax, V); c.place(vback, V); c.place(mixed, Cn); c.place(cback, Cn);
        c.place(vtile, trim_scan_tiles(nv) + 1); c.place(ftile, trim_scan_tiles(nf) + 1);
        c.place(ctile, trim_scan_tiles(3 * nf) + 1);
        c.place(vidx, V); c.place(fidx, Fn); c.place(cidx, Cn);
        c.place(counts, rep_num_words);
        c.place(out_v, 3 * (V + Cn)); c.place(out_f, Cn); c.place(origin, V + Cn);
        c.place(target, V);
    }
};

// the skeleton's device buffers, behind the field's
struct SkelScratch {
    long long sort_cap;
    int32_t *band, *ridx, *vnode, *vcnt, *voff, *ccnt, *coff, *vlist, *clist;
    unsigned int *link, *changed, *nflags;
    uint8_t *is_root, *rim;
    long long *rtile, *tile;
    unsigned long long *sortbuf, *scan_counts, *n_out;
    double *area3, *rec;                   // rec: ten words a node

    void lay(Carve& c, int64_t nv, int64_t nf)
    {
        const size_t V = (size_t)nv, Cn = 3 * (size_t)nf;
        sort_cap = geo_sort_size(std::max<long long>(nv, 3 * nf));
        c.place(band, V); c.place(link, V); c.place(changed, 1); c.place(is_root, V);
        c.place(ridx, V); c.place(rtile, trim_scan_tiles(nv) + 1); c.place(sortbuf, (size_t)sort_cap);
        c.place(vnode, V); c.place(rim, V); c.place(nflags, V); c.place(vcnt, V);
        c.place(voff, V + 1); c.place(ccnt, V); c.place(coff, V + 1);
        c.place(tile, mesh_csr_tiles(nv) + 1); c.place(scan_counts, 4); c.place(vlist, V);
        c.place(clist, Cn); c.place(area3, (size_t)nf); c.place(rec, 10 * V); c.place(n_out, 1);
    }
};

// the geodesic field: the adjacency, one weight per adjacency entry, the seed bytes, the two flag arrays, the marks of a
// batch of n_marks rounds, [dist | pred | counters] -- one range of field_down() bytes for the download, which is why
// their offsets keep their names -- and, for the skeleton, what SkelScratch lists
struct FieldScratch {
    CsrDev d;
    SkelScratch sk;
    size_t o_dist, o_pred, o_counts;
    double* w;
    uint8_t* is_seed;
    unsigned int *flag_a, *flag_b;
    unsigned long long *marks, *dist, *counts;
    int32_t* pred;

    void lay(Carve& c, int64_t nv, int64_t nf, size_t n_marks, bool skeleton)
    {
        const size_t V = (size_t)nv, n_blocks = geo_blocks(nv);
        d.lay(c, nf, nv);
        c.place(w, 6 * (size_t)nf); c.place(is_seed, V); c.place(flag_a, n_blocks);
        c.place(flag_b, n_blocks); c.place(marks, n_marks);
        o_dist = c.place(dist, V); o_pred = c.place(pred, V); o_counts = c.place(counts, geo_num_words);
        if (skeleton) sk.lay(c, nv, nf);
    }
    size_t field_down() const { return o_counts + geo_num_words * 8 - o_dist; }
};

}  // namespace mm
