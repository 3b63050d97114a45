// The fit of csrc/mm_bspline_fit.h compiled for the CPU (tests/test_bspline_fit_host.py): one contour in, what the
// kernel of mm_bspline_kernels.hip writes for it out.  guard doubles behind the work arrays must stay untouched.
#include <cmath>
#include <vector>

#include "mm_bspline_fit.h"

using namespace mm::bspl;

extern "C" int bspline_fit_host(const double* pts, int m, int k, double s, double* out, double* fp, int* nknots,
                                int* guard_ok)
{
    const size_t wd = work_doubles(m, k), guard = 64;
    std::vector<double> ws(wd + guard, -777.0);
    Work w;
    carve(ws.data(), m, k, w);
    int n = 0;
    double f = 0.0;
    int st = fit(pts, m, k, s, w, n, f);
    const bool curve = st == kFitted || st == kInterpolated || st == kCollapsed || st == kIterationLimit;
    bool bad = !std::isfinite(f);
    if (curve) {
        for (int i = 0; i < m; ++i) {
            if (!evaluate(w.t, w.c, n, k, m, i, out + 3 * i)) bad = true;
            for (int d = 0; d < 3; ++d) bad = bad || !std::isfinite(out[3 * i + d]);
        }
        if (bad) st = kUnchangedNonFinite;
    }
    *fp = f;
    *nknots = curve && !bad ? n : 0;
    *guard_ok = 1;
    for (size_t i = wd; i < wd + guard; ++i)
        if (ws[i] != -777.0) *guard_ok = 0;
    return st;
}
