// The carve arithmetic of csrc/mm_stage.h and the record layouts of csrc/mm_point_records.h on the CPU, no GPU and no
// engine: StagedPass is placed over two heap blocks of exactly the sizes reserve() asks the engine for, and every
// carved region is written end to end through the pointers the wrappers use, so a sanitizer build sees any region that
// leaves its block or overlaps its neighbour.  Sizes: empty and odd ones around the 256-byte step.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mm_stage.h"

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

int main()
{
    const size_t sizes[] = {0, 1, 255, 256, 257};
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
