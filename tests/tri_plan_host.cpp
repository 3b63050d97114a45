// csrc/mm_tri_plan.h on the CPU, a program of its own (tests/test_relax_host.py builds it plain and under the address
// and undefined-behaviour sanitizers and runs it directly): the argument checks, the plan of a small tube -- both
// permutations, the item count, the chunk boxes, every bound against the nearest corner of its item -- and the staged
// records.  The header reaches the engine's declarations through mm_stage.h; the three functions it calls from the
// library are stood in for here, nothing of the GPU runtime is called.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "mm_tri_plan.h"

namespace mm {
static std::string g_last;
int set_error(int code, const std::string& msg) { g_last = msg; return code; }
int tri_queries_per_block() { return 512; }
int tri_chunk_faces() { return 256; }
}  // namespace mm

using namespace mm;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

int main()
{
    // an open tube: n_around x n_rings vertices, two triangles a quad
    const int n_around = 12, n_rings = 60;
    std::vector<double> v;
    std::vector<int64_t> f;
    for (int r = 0; r < n_rings; ++r)
        for (int a = 0; a < n_around; ++a) {
            const double t = 2.0 * 3.14159265358979323846 * a / n_around;
            v.push_back(std::cos(t)); v.push_back(std::sin(t)); v.push_back(0.25 * r);
        }
    for (int r = 0; r + 1 < n_rings; ++r)
        for (int a = 0; a < n_around; ++a) {
            const int64_t i = r * n_around + a, j = r * n_around + (a + 1) % n_around;
            const int64_t quad[6] = {i, j, i + n_around, j, j + n_around, i + n_around};
            f.insert(f.end(), quad, quad + 6);
        }
    f.insert(f.end(), {0, 0, 1});                                         // a degenerate face
    for (int k = 0; k < 3; ++k) v.push_back(0.5 * (v[(size_t)k] + v[(size_t)(3 + k)]) + (k == 2 ? 0x1p-25 : 0.0));
    f.insert(f.end(), {0, 1, (int64_t)v.size() / 3 - 1});                 // a thin face: a cap of height 2^-25 over 0 - 1
    const int64_t nv = (int64_t)v.size() / 3, nf = (int64_t)f.size() / 3;
    std::vector<double> q;
    for (int64_t i = 0; i < nv; ++i)
        for (int k = 0; k < 3; ++k) q.push_back(v[(size_t)(3 * i + k)] * (k < 2 ? 1.1 : 1.0) + 0.01 * ((i * 7 + k) % 5));
    const int64_t nq = nv;

    CHECK(plan_args(v.data(), nv, f.data(), nf, q.data(), nq, "t") == MM_OK);
    std::vector<double> bad = v;
    bad[4] = std::numeric_limits<double>::infinity();
    CHECK(plan_args(bad.data(), nv, f.data(), nf, q.data(), nq, "t") == MM_ERR_INVALID && g_last.find("non-finite vertex") != std::string::npos);
    std::vector<int64_t> bad_f = f;
    bad_f[5] = nv;
    CHECK(plan_args(v.data(), nv, bad_f.data(), nf, q.data(), nq, "t") == MM_ERR_INVALID);
    CHECK(plan_args(v.data(), nv, f.data(), nf, nullptr, 0, "t") == MM_OK);
    CHECK(plan_args(v.data(), -1, f.data(), nf, q.data(), nq, "t") == MM_ERR_INVALID);

    TriPlan pl;
    CHECK(build_plan(v.data(), f.data(), nf, q.data(), nq, "t", pl) == MM_OK);
    const int64_t nqb = (nq + pl.qpb - 1) / pl.qpb, nch = (nf + pl.ch - 1) / pl.ch;
    CHECK(nqb >= 2 && nch >= 3 && pl.n_a == nqb && pl.n_b == nqb * (nch - 1));
    CHECK((int64_t)pl.work.size() == nqb * nch && (int64_t)pl.cbox.size() == nch);
    std::vector<int> seen_f((size_t)nf, 0), seen_q((size_t)nq, 0);
    for (int32_t j : pl.forder) { CHECK(j >= 0 && j < nf); if (j >= 0 && j < nf) ++seen_f[(size_t)j]; }
    for (int32_t j : pl.qperm) { CHECK(j >= 0 && j < nq); if (j >= 0 && j < nq) ++seen_q[(size_t)j]; }
    for (int c : seen_f) CHECK(c == 1);
    for (int c : seen_q) CHECK(c == 1);
    int n_degenerate = 0, n_thin = 0;
    for (uint8_t d : pl.degenerate) n_degenerate += d;
    for (uint8_t d : pl.thin) n_thin += d;
    CHECK(n_degenerate == 1 && n_thin == 1);
    for (int64_t j = 0; j < nf; ++j) CHECK(!(pl.degenerate[(size_t)j] && pl.thin[(size_t)j]));
    for (int64_t j = 0; j < nf; ++j)                                      // every corner inside its chunk's box
        for (int k = 0; k < 3; ++k) {
            const double* p = v.data() + 3 * f[(size_t)(3 * pl.forder[(size_t)j] + k)];
            const Box3& b = pl.cbox[(size_t)(j / pl.ch)];
            for (int a = 0; a < 3; ++a) CHECK(b.lo[a] <= p[a] && p[a] <= b.hi[a]);
        }
    std::vector<int> pairs((size_t)(nqb * nch), 0);
    for (const TriWork& w : pl.work) {
        CHECK(w.q0 % pl.qpb == 0 && w.c0 % pl.ch == 0 && w.q0 < nq && w.c0 < nf && w.lb2 >= 0.0);
        ++pairs[(size_t)((w.q0 / pl.qpb) * nch + w.c0 / pl.ch)];
        // no face is farther than its nearest corner: the bound stays below the nearest corner of the item
        double nearest = std::numeric_limits<double>::infinity();
        for (int64_t s = w.q0; s < std::min<int64_t>(nq, w.q0 + pl.qpb); ++s)
            for (int64_t j = w.c0; j < std::min<int64_t>(nf, w.c0 + pl.ch); ++j)
                for (int k = 0; k < 3; ++k) {
                    const double* p = q.data() + 3 * pl.qperm[(size_t)s];
                    const double* c = v.data() + 3 * f[(size_t)(3 * pl.forder[(size_t)j] + k)];
                    const double dx = p[0] - c[0], dy = p[1] - c[1], dz = p[2] - c[2];
                    nearest = std::min(nearest, (dx * dx + dy * dy) + dz * dz);
                }
        CHECK(w.lb2 <= nearest);
    }
    for (int c : pairs) CHECK(c == 1);
    for (int64_t b = 0; b < nqb; ++b)                                      // pass A holds the block's smallest bound
        for (int64_t c = 0; c + 1 < nch; ++c) CHECK(pl.work[(size_t)b].lb2 <= pl.work[(size_t)(pl.n_a + b * (nch - 1) + c)].lb2);

    std::vector<double> rec((size_t)nf * 12);
    stage_tri_records(pl, v.data(), f.data(), nf, rec.data());
    for (int64_t j = 0; j < nf; ++j) {
        unsigned long long w[3];
        for (int k = 0; k < 3; ++k) {
            std::memcpy(&w[k], &rec[(size_t)(12 * j + 4 * k + 3)], 8);
            CHECK(std::memcmp(&rec[(size_t)(12 * j + 4 * k)], v.data() + 3 * f[(size_t)(3 * pl.forder[(size_t)j] + k)], 24) == 0);
        }
        CHECK(w[0] == (pl.degenerate[(size_t)j] ? 1u : pl.thin[(size_t)j] ? 2u : 0u) && w[1] == (unsigned long long)pl.forder[(size_t)j] && w[2] == 0);
    }

    TriPlan none;
    CHECK(build_plan(v.data(), f.data(), nf, q.data(), 0, "t", none) == MM_OK && none.work.empty() && none.qperm.empty());
    CHECK(build_plan(v.data(), f.data(), 0, q.data(), nq, "t", none) == MM_OK && none.work.empty() && none.cbox.empty());
    if (failures) return 1;
    std::printf("tri_plan_host OK\n");
    return 0;
}
