// csrc/mm_winding_device.h as plain host C++, a program of its own (tests/test_winding_kernel_resources.py builds it with
// g++, plain and under the address and undefined-behaviour sanitizers, and runs it directly): the cone, the fold of
// faces and the join of partials on the octahedron of tests/winding_cases.py, where the arithmetic is exact.
#include <cmath>
#include <cstdio>
#include <vector>

#include "mm_winding_device.h"

using namespace mm::winding;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

static const double V[6][3] = {{3, 0, 0}, {-3, 0, 0}, {0, 3, 0}, {0, -3, 0}, {0, 0, 3}, {0, 0, -3}};
static const int F[8][3] = {{0, 2, 4}, {1, 4, 2}, {0, 4, 3}, {1, 3, 4}, {0, 3, 5}, {1, 5, 3}, {0, 5, 2}, {1, 2, 5}};

static void fold(State& s, const double* p, int f0, int f1, bool flip)
{
    for (int i = f0; i < f1; ++i) {
        const double *a = V[F[i][0]], *b = V[F[i][flip ? 2 : 1]], *c = V[F[i][flip ? 1 : 2]];
        face(s, p[0], p[1], p[2], a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2]);
    }
}

int main()
{
    double re = -1.0, im = 0.0;
    CHECK(cone(re, im) == 2 && re == 1.0 && im == 0.0);
    re = 1.0; im = 1.0;
    CHECK(cone(re, im) == 0 && re == 1.0 && im == 1.0);
    re = 1.0; im = 2.0;
    CHECK(cone(re, im) == 1 && re == 2.0 && im == -1.0);
    re = -1.0; im = -1.0;
    CHECK(cone(re, im) == -1 && re == 1.0 && im == -1.0);
    re = 0.5; im = -2.0;
    CHECK(cone(re, im) == -1 && re == 2.0 && im == 0.5);

    const double inside[3] = {0, 0, 0}, outside[3] = {4, 0, 0}, vertex[3] = {3, 0, 0}, on_face[3] = {1, 1, 1};
    State s = start();
    fold(s, inside, 0, 8, false);
    CHECK(s.n == 4 && s.pi == 0.0 && s.pr >= 0.5 && s.pr < 1.0 && !s.touch && s.rho == 1.0);
    s = start();
    fold(s, inside, 0, 8, true);
    CHECK(s.n == -4 && s.pi == 0.0);
    s = start();
    fold(s, outside, 0, 8, false);
    CHECK(s.n == 0 && s.pi == 0.0 && !s.touch && s.rho > 0.0);
    // two partials joined give the angle of the whole
    State a = start(), b = start();
    fold(a, outside, 0, 3, false);
    fold(b, outside, 3, 8, false);
    join(a, b);
    CHECK(a.n == 0 && a.rho == s.rho && std::fabs(a.pi) <= 0x1p-50 * a.pr);
    s = start();
    fold(s, vertex, 0, 8, false);
    CHECK(s.rho == 0.0);
    s = start();
    fold(s, on_face, 0, 8, false);
    CHECK(s.touch == 1);
    if (!failures) std::printf("winding_device_host OK\n");
    return failures ? 1 : 0;
}
