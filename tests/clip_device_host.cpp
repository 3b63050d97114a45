// csrc/mm_clip_device.h as plain host C++, a program of its own (tests/test_clip_kernel_resources.py builds it with g++,
// plain and under the address and undefined-behaviour sanitizers, and runs it directly): rule C4 on fixed faces whose
// arithmetic is exact -- the rotation to every apex, both diagonals and the tie, the kept pieces under every drop
// pattern, null pieces where a loop point lies on a vertex; C2's orphan test at every apex, kept and not.
#include <cstdio>

#include "mm_clip_device.h"

using namespace mm::clip;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static bool is(const Piece& p, int i0, int i1, int i2) { return p.i0 == i0 && p.i1 == i1 && p.i2 == i2; }

int main()
{
    static_assert(sizeof(Record) == 48, "record");
    // the face (10, 11, 12) in the plane z = 0; loop points 20 (on a-b) and 21 (on c-a)
    const Corner v0{10, {0, 0, 0}, false}, v1{11, {4, 0, 0}, false}, v2{12, {0, 4, 0}, false};

    // apex 0: a = 10, b = 11, c = 12; m_ab = (1, 0, 0), m_ca = (0, 2, 0): |m_ab - c|^2 = 17 < |b - m_ca|^2 = 20, through c
    {
        const Corner mab{20, {1, 0, 0}, false}, mca{21, {0, 2, 0}, false};
        CHECK(sq_dist(mab.p, v2.p) == 17.0 && sq_dist(v1.p, mca.p) == 20.0);
        const Pieces p = face_pieces(v0, v1, v2, 0, mab, mca);
        CHECK(is(p.apex, 10, 20, 21) && is(p.first, 20, 11, 12) && is(p.second, 20, 12, 21));
        CHECK(p.apex.kept && p.first.kept && p.second.kept && !p.apex.null && !p.first.null && !p.second.null);
    }
    // the other diagonal: m_ab = (3, 0, 0), m_ca = (0, 1, 0): 25 against 17
    {
        const Corner mab{20, {3, 0, 0}, false}, mca{21, {0, 1, 0}, false};
        const Pieces p = face_pieces(v0, v1, v2, 0, mab, mca);
        CHECK(is(p.apex, 10, 20, 21) && is(p.first, 20, 11, 21) && is(p.second, 11, 12, 21));
    }
    // a tie goes to b - m_ca: m_ab = (2, 0, 0), m_ca = (0, 2, 0): 20 against 20
    {
        const Corner mab{20, {2, 0, 0}, false}, mca{21, {0, 2, 0}, false};
        CHECK(sq_dist(mab.p, v2.p) == sq_dist(v1.p, mca.p));
        const Pieces p = face_pieces(v0, v1, v2, 0, mab, mca);
        CHECK(is(p.first, 20, 11, 21) && is(p.second, 11, 12, 21));
    }
    // the rotation keeps the winding: apex 1 -> (11, 12, 10), apex 2 -> (12, 10, 11)
    {
        const Corner mab{20, {2, 2, 0}, false}, mca{21, {3, 0, 0}, false};          // on 11-12 and on 10-11
        const Pieces p = face_pieces(v0, v1, v2, 1, mab, mca);
        CHECK(is(p.apex, 11, 20, 21));
        CHECK((is(p.first, 20, 12, 10) && is(p.second, 20, 10, 21)) || (is(p.first, 20, 12, 21) && is(p.second, 12, 10, 21)));
        const Corner nab{20, {0, 3, 0}, false}, nca{21, {1, 3, 0}, false};          // on 12-10 and on 11-12
        const Pieces q = face_pieces(v0, v1, v2, 2, nab, nca);
        CHECK(is(q.apex, 12, 20, 21) && q.first.i0 == 20 && q.first.i1 == 10 && q.second.i2 == 21);
    }
    // dropped vertices: the apex piece hangs on a alone, the quad's pieces on b and c as they hold them
    {
        const Corner mab{20, {1, 0, 0}, false}, mca{21, {0, 2, 0}, false};          // through c: (m_ab, b, c), (m_ab, c, m_ca)
        const Corner d0{-1, v0.p, true}, d1{-1, v1.p, true}, d2{-1, v2.p, true};
        Pieces p = face_pieces(d0, v1, v2, 0, mab, mca);
        CHECK(!p.apex.kept && p.first.kept && p.second.kept);
        p = face_pieces(v0, d1, d2, 0, mab, mca);
        CHECK(p.apex.kept && !p.first.kept && !p.second.kept);
        p = face_pieces(v0, d1, v2, 0, mab, mca);
        CHECK(p.apex.kept && !p.first.kept && p.second.kept);
        const Corner nab{20, {3, 0, 0}, false}, nca{21, {0, 1, 0}, false};          // through b: (m_ab, b, m_ca), (b, c, m_ca)
        p = face_pieces(v0, v1, d2, 0, nab, nca);
        CHECK(p.apex.kept && p.first.kept && !p.second.kept);
    }
    // a plane through vertex b: m_ab has b's coordinates; the piece that holds both is null and is still a piece
    {
        const Corner mab{20, {4, 0, 0}, false}, mca{21, {0, 2, 0}, false};
        const Pieces p = face_pieces(v0, v1, v2, 0, mab, mca);
        CHECK(!p.apex.null && p.first.null && p.first.kept && !p.second.null);
        CHECK(same_point(mab.p, v1.p) && !same_point(mab.p, mca.p));
    }
    CHECK(rim_runs_ab_to_ca(kApexKept | 1) && !rim_runs_ab_to_ca(kLoopCut | kClosedRim | 2));
    // the orphan test: apex kept -> the apex alone decides; apex dropped -> either of the other two
    for (int apex = 0; apex < 3; ++apex)
        for (int d = 0; d < 8; ++d) {
            const bool d0 = d & 1, d1 = d & 2, d2 = d & 4;
            const bool da = apex == 0 ? d0 : (apex == 1 ? d1 : d2);
            const int others = (d0 + d1 + d2) - da;
            CHECK(kept_side_dropped(apex | kApexKept | kLoopCut, d0, d1, d2) == da);
            CHECK(kept_side_dropped(apex | kClosedRim, d0, d1, d2) == (others > 0));
        }
    if (failures) return 1;
    std::printf("clip_device_host OK\n");
    return 0;
}
