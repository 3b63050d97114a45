// The carve arithmetic of csrc/mm_stage.h and the record layouts of csrc/mm_point_records.h on the CPU, no GPU and no
// engine: StagedPass is placed over two heap blocks of exactly the sizes reserve() asks the engine for, and every
// carved region is written end to end through the pointers the wrappers use, so a sanitizer build sees any region that
// leaves its block or overlaps its neighbour.  Sizes: empty and odd ones around the 256-byte step.  The typed carving
// (Carve::place) the same way, against take(); and the layouts of csrc/mm_mesh_layout.h against recorded sizes and offsets.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mm_mesh_layout.h"

using namespace mm;

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

template <class T> static void fill(T* p, size_t bytes, unsigned char v)
{
    std::memset((void*)p, v, bytes);
}

static int one_pass(size_t a, size_t b, size_t c, size_t s)
{
    StagedPass sp;
    const size_t o_a = sp.in.take(a), o_b = sp.in.take(b * sizeof(BranchClPoint));
    const size_t o_c = sp.out.take(c * sizeof(NnWork)), o_d = sp.out.take(a);
    const size_t o_s = sp.scratch.take(s * sizeof(RayPartial));
    CHECK(o_a == 0 && o_c == 0 && o_s == 0);
    CHECK(o_b == up256(a) && o_d == up256(c * sizeof(NnWork)));
    CHECK(sp.in.size() % 256 == 0 && sp.out.size() % 256 == 0 && sp.scratch.size() % 256 == 0);
    CHECK(sp.in.size() >= o_b + b * sizeof(BranchClPoint) && sp.out.size() >= o_d + a);
    // the two blocks StagedPass::reserve() asks for, at the alignment hipMalloc / hipHostMalloc give at the least
    const size_t host_bytes = std::max(sp.in.size(), sp.out.size());
    const size_t dev_bytes = sp.in.size() + sp.out.size() + sp.scratch.size();
    sp.h = (unsigned char*)std::aligned_alloc(256, host_bytes ? host_bytes : 256);
    sp.d = (unsigned char*)std::aligned_alloc(256, dev_bytes ? dev_bytes : 256);
    CHECK(sp.h && sp.d);
    fill(sp.host<unsigned char>(o_a), a, 1);
    fill(sp.host<BranchClPoint>(o_b), b * sizeof(BranchClPoint), 2);
    CHECK((size_t)sp.host<BranchClPoint>(o_b) % alignof(BranchClPoint) == 0);
    fill(sp.dev_in<unsigned char>(o_a), a, 3);
    fill(sp.dev_in<BranchClPoint>(o_b), b * sizeof(BranchClPoint), 4);
    fill(sp.dev_out<NnWork>(o_c), c * sizeof(NnWork), 5);
    fill(sp.dev_out<unsigned char>(o_d), a, 6);
    fill(sp.dev_scratch<RayPartial>(o_s), s * sizeof(RayPartial), 7);
    CHECK((size_t)sp.dev_in<BranchClPoint>(o_b) % alignof(BranchClPoint) == 0);
    CHECK((size_t)sp.dev_out<NnWork>(o_c) % alignof(NnWork) == 0);
    CHECK((size_t)sp.dev_scratch<RayPartial>(o_s) % alignof(RayPartial) == 0);
    // the regions are disjoint: each still holds its own fill
    for (size_t i = 0; i < a; ++i) CHECK(sp.dev_in<unsigned char>(o_a)[i] == 3 && sp.dev_out<unsigned char>(o_d)[i] == 6);
    for (size_t i = 0; i < b * sizeof(BranchClPoint); ++i) CHECK(sp.dev_in<unsigned char>(o_b)[i] == 4);
    for (size_t i = 0; i < c * sizeof(NnWork); ++i) CHECK(sp.dev_out<unsigned char>(o_c)[i] == 5);
    for (size_t i = 0; i < s * sizeof(RayPartial); ++i) CHECK(sp.dev_scratch<unsigned char>(o_s)[i] == 7);
    // the download: the output tail of the device block over the start of the host block
    std::memcpy(sp.h, sp.d + sp.in.size(), sp.out.size());
    for (size_t i = 0; i < c * sizeof(NnWork); ++i) CHECK(sp.host<unsigned char>(o_c)[i] == 5);
    for (size_t i = 0; i < a; ++i) CHECK(sp.host<unsigned char>(o_d)[i] == 6);
    std::free(sp.h);
    std::free(sp.d);
    return 0;
}

// ---- typed carving: place() against take(), measuring against placing, the regions written through their pointers ----

struct Four {
    uint8_t* bytes; double* reals; TriWork* items; int32_t* ints;
    size_t at[4];
    void lay(Carve& c, size_t a, size_t b, size_t n)
    {
        at[0] = c.place(bytes, a); at[1] = c.place(reals, b); at[2] = c.place(items, n); at[3] = c.place(ints, a);
    }
};

static int one_carve(size_t a, size_t b, size_t n)
{
    Carve ref;
    const size_t want[4] = {ref.take(a), ref.take(b * sizeof(double)), ref.take(n * sizeof(TriWork)), ref.take(a * sizeof(int32_t))};
    Four m, p;
    Carve measure;
    m.lay(measure, a, b, n);
    CHECK(measure.size() == ref.size());
    CHECK(!m.bytes && !m.reals && !m.items && !m.ints);                 // measuring places nothing
    unsigned char* block = (unsigned char*)std::aligned_alloc(256, measure.size() ? measure.size() : 256);
    CHECK(block);
    Carve c{block};
    p.lay(c, a, b, n);
    CHECK(c.size() == measure.size());
    for (int k = 0; k < 4; ++k) CHECK(m.at[k] == want[k] && p.at[k] == want[k]);
    CHECK((unsigned char*)p.bytes == block + want[0] && (unsigned char*)p.reals == block + want[1]);
    CHECK((unsigned char*)p.items == block + want[2] && (unsigned char*)p.ints == block + want[3]);
    CHECK((size_t)p.reals % alignof(double) == 0 && (size_t)p.items % alignof(TriWork) == 0 && (size_t)p.ints % alignof(int32_t) == 0);
    // end to end through the typed pointers, then each region still holds its own fill: disjoint and inside the block
    for (size_t i = 0; i < a; ++i) p.bytes[i] = 1;
    for (size_t i = 0; i < b; ++i) std::memset(&p.reals[i], 2, sizeof(double));
    for (size_t i = 0; i < n; ++i) std::memset(&p.items[i], 3, sizeof(TriWork));
    for (size_t i = 0; i < a; ++i) std::memset(&p.ints[i], 4, sizeof(int32_t));
    CHECK(want[3] + a * sizeof(int32_t) <= measure.size());
    for (size_t i = 0; i < a; ++i) CHECK(block[want[0] + i] == 1);
    for (size_t i = 0; i < b * sizeof(double); ++i) CHECK(block[want[1] + i] == 2);
    for (size_t i = 0; i < n * sizeof(TriWork); ++i) CHECK(block[want[2] + i] == 3);
    for (size_t i = 0; i < a * sizeof(int32_t); ++i) CHECK(block[want[3] + i] == 4);
    std::free(block);
    return 0;
}

// ---- the layouts of mm_mesh_layout.h against the sizes and offsets their hand-written predecessors had ----

// the sizes the kernel files export (kMeshThreads = 256 lanes, kScanTile = 4096 items), restated for a program without them
namespace mm {
size_t trim_scan_tiles(long long n) { return (size_t)((n + 4095) / 4096); }
size_t mesh_csr_tiles(long long n) { return (size_t)((n + 4095) / 4096); }
size_t refine_tiles(long long n) { return (size_t)((n + 4095) / 4096); }
size_t weld_sum_scratch(long long nf) { return (size_t)((nf + 255) / 256) + 1; }
size_t geo_blocks(long long nv) { return (size_t)((nv + 255) / 256); }
long long geo_sort_size(long long n) { long long p = 2; while (p < n) p <<= 1; return p; }
}  // namespace mm

// {total size, first buffer behind the edge table / the adjacency, last buffer, counters}; the field, whose counters are
// its last buffer: {size, w, counters, dist}.  Recorded from commit 9f96ef1, the last with the layouts written out as
// o_* fields in mm_flip, mm_collapse, mm_refine, mm_repair and mm_geodesic .cpp.  (30, 42) and (30, 43) straddle the
// table's growth from 2^8 to 2^9 slots (6 * 43 > 256); (5000, 9996) passes the 4096-item scan and adjacency tiles.
struct Recorded {
    long long nv, nf;
    size_t flip[4], collapse[4], refine[4], refine_list[4], repair[4], field[4], skeleton[4];
};
static const Recorded kRecorded[] = {
    {1, 1, {11520, 5120, 11264, 10752}, {16384, 5120, 16128, 10752}, {6912, 5120, 6912, 6144}, {7424, 5120, 6912, 6144},
     {19712, 5120, 19456, 18432}, {8192, 5888, 7936, 7424}, {13568, 8192, 13312, 7936}},
    {4, 4, {11520, 5120, 11264, 10752}, {16384, 5120, 16128, 10752}, {6912, 5120, 6912, 6144}, {7424, 5120, 6912, 6144},
     {19968, 5120, 19712, 18432}, {8192, 5888, 7936, 7424}, {13824, 8192, 13568, 7936}},
    {30, 42, {11776, 5120, 11520, 10752}, {17408, 5120, 17152, 10752}, {7424, 5120, 7424, 6400}, {9472, 5120, 7424, 6400},
     {25344, 5120, 25088, 19712}, {9984, 5888, 9728, 9216}, {18944, 9984, 18688, 9728}},
    {30, 43, {22016, 10240, 21760, 20992}, {28928, 10240, 28672, 20992}, {12800, 10240, 12800, 11776}, {15360, 10240, 12800, 11776},
     {37888, 10240, 37632, 32000}, {15360, 11008, 15104, 14592}, {25600, 15360, 25344, 15104}},
    {5000, 9996, {2762752, 1310720, 2762240, 2681856}, {3442944, 1310720, 3442432, 2681856}, {1562368, 1310720, 1562368, 1481472},
     {2042624, 1310720, 1562368, 1481472}, {4999424, 1310720, 4979200, 3878912}, {1898240, 1351424, 1897984, 1837568},
     {2974464, 1898240, 2974208, 1897984}},
};

// lay measured and placed over a block of exactly that size; first, last, counters: the three pointers to compare
template <class Lay, class Pick> static int one_layout(const size_t want[4], Lay lay, Pick pick)
{
    Carve measure;
    lay(measure);
    CHECK(measure.size() == want[0]);
    unsigned char* block = (unsigned char*)std::aligned_alloc(256, measure.size());
    CHECK(block);
    Carve c{block};
    lay(c);
    CHECK(c.size() == want[0]);
    const void* at[3];
    if (pick(at)) return 1;
    for (int k = 0; k < 3; ++k) CHECK((size_t)((const unsigned char*)at[k] - block) == want[k + 1]);
    std::free(block);
    return 0;
}

static int layouts()
{
    for (const Recorded& r : kRecorded) {
        const long long nv = r.nv, nf = r.nf;
        FlipScratch f;
        if (one_layout(r.flip, [&](Carve& c) { f.lay(c, nv, nf); },
                       [&](const void** at) -> int {
                           at[0] = f.first; at[1] = f.sb; at[2] = f.counts;
                           CHECK((unsigned char*)f.t.cnt - (unsigned char*)f.t.keys == (ptrdiff_t)(f.t.slots() * 8));
                           CHECK((unsigned char*)f.t.own - (unsigned char*)f.t.cnt == (ptrdiff_t)(f.t.slots() * 4));
                           return 0;
                       })) return 1;
        CollapseScratch s;
        if (one_layout(r.collapse, [&](Carve& c) { s.lay(c, nv, nf); },
                       [&](const void** at) -> int { at[0] = s.first; at[1] = s.sb; at[2] = s.counts; return 0; })) return 1;
        RefineScratch p;
        if (one_layout(r.refine, [&](Carve& c) { p.lay(c, nf); },
                       [&](const void** at) -> int { at[0] = p.slot; at[1] = p.list; at[2] = p.counts; return 0; })) return 1;
        const size_t list_bytes = up256((size_t)nf * 24) + (size_t)nf * 24;           // what mm_mesh_edge_lengths asks for
        if (one_layout(r.refine_list, [&](Carve& c) { p.lay(c, nf, list_bytes); },
                       [&](const void** at) -> int { at[0] = p.slot; at[1] = p.list; at[2] = p.counts; return 0; })) return 1;
        RepairScratch q;
        if (one_layout(r.repair, [&](Carve& c) { q.lay(c, nv, nf); },
                       [&](const void** at) -> int { at[0] = q.rep; at[1] = q.target; at[2] = q.counts; return 0; })) return 1;
        FieldScratch g;
        const size_t kMarks = 64;                                      // the longest batch of mm_geodesic.cpp
        if (one_layout(r.field, [&](Carve& c) { g.lay(c, nv, nf, kMarks, false); },
                       [&](const void** at) -> int {
                           at[0] = g.w; at[1] = g.counts; at[2] = g.dist;
                           CHECK(g.d.nb == (int32_t*)g.d.edges.own);   // the rows lie over the owner words
                           CHECK(g.field_down() == (size_t)((unsigned char*)g.counts - (unsigned char*)g.dist) + geo_num_words * 8);
                           return 0;
                       })) return 1;
        if (one_layout(r.skeleton, [&](Carve& c) { g.lay(c, nv, nf, kMarks, true); },
                       [&](const void** at) -> int { at[0] = g.sk.band; at[1] = g.sk.n_out; at[2] = g.counts; return 0; })) return 1;
    }
    return 0;
}

int main()
{
    const size_t sizes[] = {0, 1, 255, 256, 257};
    for (size_t a : sizes)
        for (size_t b : sizes)
            for (size_t n : sizes)
                if (one_carve(a, b, n)) return 1;
    if (layouts()) return 1;
    for (size_t v : sizes) {
        Carve c;
        CHECK(c.take(v) == 0 && c.size() == (v + 255) / 256 * 256);
        const size_t end = c.size(), at0 = c.take(0), at1 = c.take(1);
        CHECK(at0 == end && at1 == end && c.size() == end + 256);
    }
    for (size_t a : sizes)
        for (size_t b : sizes)
            for (size_t c : sizes)
                if (one_pass(a, b, c, (a + c) % 5)) return 1;
    // block work lists: none for an empty job or an empty set, one per started block otherwise
    const int64_t pt_off[] = {0, 0, 255, 511, 768, 769}, set_off[] = {0, 3, 3, 5, 6, 7};
    std::vector<PointWork> work;
    const double evals = point_blocks(5, pt_off, set_off, 256, work);
    CHECK(work.size() == 4 && work[0].job == 2 && work[0].p0 == 0 && work[1].job == 3 && work[1].p0 == 0);
    CHECK(work[2].job == 3 && work[2].p0 == 256 && work[3].job == 4 && work[3].p0 == 0);
    CHECK(evals == 256.0 * 2 + 257.0 + 1.0);
    std::printf("stage_host OK\n");
    return 0;
}
