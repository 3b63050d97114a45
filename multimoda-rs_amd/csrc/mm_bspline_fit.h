// mm_bspline_fit.h -- the closed smoothing B-spline of one contour (Dierckx's closed-curve algorithm, the one behind
// scipy's splprep(per=True)), written once for the kernel of mm_bspline_kernels.hip.  Everything is
// f64 in one fixed operation order and never fused (the build passes -ffp-contract=off): tests/mm_checkers/bspline.py
// states the same arithmetic statement for statement and the two agree bit for bit.  Indices are 1-based like the
// published algorithm, through the accessor macros below; the guards for tiny systems (fewer interior knots than border
// columns) then read as in the book.  Every division goes through dv(): a zero divisor marks the system singular and
// the contour comes back unchanged.
#pragma once

#include <cmath>
#include <cstdint>

#ifndef MM_HD
#if defined(__HIPCC__)
#define MM_HD __host__ __device__ inline
#else
#define MM_HD inline
#endif
#endif

namespace mm {
namespace bspl {

enum Status : int32_t {
    kFitted = 0, kInterpolated = 1, kCollapsed = 2, kUnchangedShort = 3, kUnchangedZeroChord = 4,
    kUnchangedNonFinite = 5, kIterationLimit = 6
};
constexpr int kDim = 3;
constexpr int kMaxDegree = 5;
constexpr int kMaxIter = 20;
constexpr double kTol = 1e-3;

// The arrays of one contour (m points, degree k, nest = m + 2k knots at the most), carved from one block of doubles.
struct Work {
    double *x, *u, *t, *fpint, *z, *c, *a1, *a2, *b, *g1, *g2, *q;
    int32_t* nrdata;
};

MM_HD size_t work_doubles(int m, int k)
{
    const size_t N = (size_t)m + 2 * (size_t)k, k1 = (size_t)k + 1, k2 = (size_t)k + 2;
    // x 3m, u m, t N+1, fpint N+1, z 3N, c 3N, a1 N k1, a2 N k, b N k2, g1 N k2, g2 N k1, q m k1, nrdata (N+2)/2
    return 3 * (size_t)m + m + 2 * (N + 1) + 6 * N + N * (k1 + k + k2 + k2 + k1) + (size_t)m * k1 + (N + 2) / 2 + 1;
}

MM_HD void carve(double* base, int m, int k, Work& w)
{
    const size_t N = (size_t)m + 2 * (size_t)k, k1 = (size_t)k + 1, k2 = (size_t)k + 2;
    double* p = base;
    w.x = p; p += 3 * (size_t)m;
    w.u = p; p += m;
    w.t = p; p += N + 1;
    w.fpint = p; p += N + 1;
    w.z = p; p += 3 * N;
    w.c = p; p += 3 * N;
    w.a1 = p; p += N * k1;
    w.a2 = p; p += N * k;
    w.b = p; p += N * k2;
    w.g1 = p; p += N * k2;
    w.g2 = p; p += N * k1;
    w.q = p; p += (size_t)m * k1;
    w.nrdata = (int32_t*)p;
}

MM_HD double dv(double a, double b, int& sing)
{
    if (b == 0.0) sing = 1;
    return a / b;
}

MM_HD void givens(double piv, double& ww, double& cs, double& sn, int& sing)
{
    const double store = std::fabs(piv);
    double dd;
    if (store >= ww) { const double r = dv(ww, piv, sing); dd = store * std::sqrt(1.0 + r * r); }
    else             { const double r = dv(piv, ww, sing); dd = ww * std::sqrt(1.0 + r * r); }
    cs = dv(ww, dd, sing);
    sn = dv(piv, dd, sing);
    ww = dd;
}

// a = cs a - sn b, b = cs b + sn a (both from the old values)
MM_HD void rota(double cs, double sn, double& a, double& b)
{
    const double av = a, bv = b;
    b = cs * bv + sn * av;
    a = cs * av - sn * bv;
}

#define T_(i) t[(i) - 1]
#define U_(i) u[(i) - 1]

// the k + 1 B-splines of degree k that are non-zero on t(l) <= x < t(l + 1), into h[1..k+1]
MM_HD void bspl(const double* t, int k, double x, int l, double* h, int& sing)
{
    double hh[kMaxDegree + 2];
    h[1] = 1.0;
    for (int j = 1; j <= k; ++j) {
        for (int i = 1; i <= j; ++i) hh[i] = h[i];
        h[1] = 0.0;
        for (int i = 1; i <= j; ++i) {
            const int li = l + i, lj = li - j;
            if (T_(li) == T_(lj)) { h[i + 1] = 0.0; continue; }
            const double f = dv(hh[i], T_(li) - T_(lj), sing);
            h[i] = h[i] + f * (T_(li) - x);
            h[i + 1] = f * (x - T_(lj));
        }
    }
}

// solve | a ' b | c = z: a upper band (wa columns stored, k + 1 used) on rows 1..n-k, b (wb columns stored) the last k
// columns.  z and c may be the same array.
MM_HD void back_periodic(const double* a, int wa, const double* b, int wb, const double* z, int n, int k, double* c,
                         int& sing)
{
#define A_(i, j) a[((i) - 1) * wa + (j) - 1]
#define B_(i, j) b[((i) - 1) * wb + (j) - 1]
    const int n2 = n - k;
    int l = n;
    for (int i = 1; i <= k; ++i) {
        double store = z[l - 1];
        const int j = k + 2 - i;
        if (i != 1) {
            int l0 = l;
            for (int l1 = j; l1 <= k; ++l1) { ++l0; store = store - c[l0 - 1] * B_(l, l1); }
        }
        c[l - 1] = dv(store, B_(l, j - 1), sing);
        --l;
        if (l == 0) return;
    }
    for (int i = 1; i <= n2; ++i) {
        double store = z[i - 1];
        l = n2;
        for (int j = 1; j <= k; ++j) { ++l; store = store - c[l - 1] * B_(i, j); }
        c[i - 1] = store;
    }
    int i = n2;
    c[i - 1] = dv(c[i - 1], A_(i, 1), sing);
    if (i == 1) return;
    for (int j = 2; j <= n2; ++j) {
        --i;
        double store = c[i - 1];
        const int i1 = j <= k ? j - 1 : k;
        l = i;
        for (int l0 = 1; l0 <= i1; ++l0) { ++l; store = store - c[l - 1] * A_(i, l0 + 1); }
        c[i - 1] = dv(store, A_(i, 1), sing);
    }
#undef A_
#undef B_
}

// The fit of one contour by ONE thread: pts = m xyz triples (finite, m >= k + 1, 1 <= k <= 5, s >= 0 finite).
// Returns the status; on a fitted / interpolated / collapsed / iteration-limit status w.t[0..n) are the knots and
// w.c the three coefficient blocks of n each.  kUnchangedNonFinite stands for a singular system here.
MM_HD int32_t fit(const double* pts, int m, int k, double s, Work& w, int& n_out, double& fp_out)
{
    double *x = w.x, *u = w.u, *t = w.t, *fpint = w.fpint, *z = w.z, *c = w.c;
    double *a1 = w.a1, *a2 = w.a2, *b = w.b, *g1 = w.g1, *g2 = w.g2, *q = w.q;
    int32_t* nrdata = w.nrdata;
    const int k1 = k + 1, k2 = k + 2;
#define X_(i) x[(i) - 1]
#define Z_(i) z[(i) - 1]
#define C_(i) c[(i) - 1]
#define FP_(i) fpint[(i) - 1]
#define NR_(i) nrdata[(i) - 1]
#define A1_(i, j) a1[((i) - 1) * k1 + (j) - 1]
#define A2_(i, j) a2[((i) - 1) * k + (j) - 1]
#define BB_(i, j) b[((i) - 1) * k2 + (j) - 1]
#define G1_(i, j) g1[((i) - 1) * k2 + (j) - 1]
#define G2_(i, j) g2[((i) - 1) * k1 + (j) - 1]
#define Q_(i, j) q[((i) - 1) * k1 + (j) - 1]
    int sing = 0;
    n_out = 0;
    fp_out = 0.0;
    // the last point gives way to the first; chord-length parameter over the modified points
    for (int i = 0; i < m; ++i) {
        const int src = i == m - 1 ? 0 : i;
        for (int d = 0; d < kDim; ++d) x[kDim * i + d] = pts[kDim * src + d];
    }
    U_(1) = 0.0;
    for (int i = 2; i <= m; ++i) {
        double dist = 0.0;
        for (int d = 1; d <= kDim; ++d) {
            const double dd = X_(kDim * (i - 1) + d) - X_(kDim * (i - 2) + d);
            dist = dist + dd * dd;
        }
        U_(i) = U_(i - 1) + std::sqrt(dist);
    }
    if (!(U_(m) > 0.0)) return kUnchangedZeroChord;
    const double total = U_(m);
    if (!std::isfinite(total)) return kUnchangedNonFinite;      // finite coordinates whose squared chord overflows
    for (int i = 2; i <= m; ++i) U_(i) = U_(i) / total;
    U_(m) = 1.0;
    for (int i = 2; i <= m; ++i) {
        if (!std::isfinite(U_(i))) return kUnchangedNonFinite;
        if (U_(i - 1) >= U_(i)) return kUnchangedZeroChord;
    }

    double h[kMaxDegree + 4], h1[kMaxDegree + 4], h2[kMaxDegree + 4], xi[kDim + 1];
    const int nest = m + 2 * k, m1 = m - 1, nmin = 2 * k1, nmax = m + 2 * k;
    int kk = k, kk1 = k1;
    const double per = U_(m) - U_(1), acc = kTol * s;
    double fp0 = 0.0, fpold = 0.0, fp = 0.0, fpms = 0.0;
    int nplus = 0, n = nmin, n7 = 0, n10 = 0;

    // knots at the data parameters (odd k) or their midpoints (even k); true when the curve is already complete
    auto interpolation_knots = [&]() -> bool {
        if (k % 2 == 0) {
            for (int i = 2; i <= m1; ++i) T_(i + k) = (U_(i) + U_(i - 1)) * 0.5;
            return false;
        }
        for (int i = 2; i <= m1; ++i) T_(i + k) = U_(i);
        if (s > 0.0) return false;
        kk = k - 1; kk1 = k;
        if (kk > 0) return false;
        T_(1) = T_(m) - per;
        T_(2) = U_(1);
        T_(m + 1) = U_(m);
        T_(m + 2) = T_(3) + per;
        int jj = 0;
        for (int i = 1; i <= m1; ++i) {
            int j = i;
            for (int d = 0; d < kDim; ++d) { ++jj; C_(j) = X_(jj); j += n; }
        }
        int j = m;
        jj = 1;
        for (int d = 0; d < kDim; ++d) { C_(j) = C_(jj); j += n; jj += n; }
        return true;
    };

    if (s > 0.0 || nmax == nmin) {
        double d1 = 0.0, cs, sn;
        for (int j = 1; j <= kDim; ++j) Z_(j) = 0.0;
        int jj = 0;
        for (int it = 1; it <= m1; ++it) {
            givens(1.0, d1, cs, sn, sing);
            for (int j = 1; j <= kDim; ++j) {
                ++jj;
                double fac = 1.0 * X_(jj);
                const double zj = Z_(j);
                Z_(j) = cs * zj + sn * fac;
                fac = cs * fac - sn * zj;
                fp0 = fp0 + fac * fac;
            }
        }
        for (int j = 1; j <= kDim; ++j) Z_(j) = dv(Z_(j), d1, sing);
        fpms = fp0 - s;
        if (fpms < acc || nmax == nmin) {
            for (int i = 1; i <= k1; ++i) {
                T_(i) = U_(1) - (double)(k1 - i) * per;
                T_(i + k1) = U_(m) + (double)(i - 1) * per;
            }
            n = nmin;
            int j1 = 0;
            for (int j = 1; j <= kDim; ++j) {
                for (int i = 1; i <= k1; ++i) C_(j1 + i) = Z_(j);
                j1 += n;
            }
            n_out = n; fp_out = fp0;
            return sing ? kUnchangedNonFinite : kCollapsed;
        }
        fpold = fp0;
        nplus = 1;
        n = nmin + 1;
        const int mm = (m + 1) / 2;
        T_(k2) = U_(mm);
        NR_(1) = mm - 2;
        NR_(2) = m1 - mm;
    } else {
        n = nmax;
        if (interpolation_knots()) { n_out = n; fp_out = 0.0; return kInterpolated; }
    }

    bool part2 = false;
    while (!part2) {
        bool restart = false;
        int iter = 1;
        for (; iter <= m; ++iter) {
            if (sing) return kUnchangedNonFinite;
            int nrint = n - nmin + 1;
            T_(k1) = U_(1);
            const int nk1 = n - k1, nk2 = nk1 + 1;
            T_(nk2) = U_(m);
            for (int j = 1; j <= k; ++j) {
                T_(nk2 + j) = T_(k1 + j) + per;
                T_(k1 - j) = T_(nk2 - j) - per;
            }
            const int nc = kDim * n;
            for (int i = 1; i <= nc; ++i) Z_(i) = 0.0;
            for (int i = 1; i <= nk1; ++i)
                for (int j = 1; j <= kk1; ++j) A1_(i, j) = 0.0;
            n7 = nk1 - k;
            n10 = n7 - kk;
            int jper = 0;
            fp = 0.0;
            int l = k1, jj = 0;
            double cs, sn;
            for (int it = 1; it <= m1; ++it) {
                if (sing) return kUnchangedNonFinite;
                const double ui = U_(it);
                for (int j = 1; j <= kDim; ++j) { ++jj; xi[j] = X_(jj); }
                while (!(ui < T_(l + 1)) && l < nk1) ++l;
                bspl(t, k, ui, l, h, sing);
                for (int i = 1; i <= k1; ++i) Q_(it, i) = h[i];
                const int l5 = l - k1;
                if (l5 < n10) {
                    // a row that touches no border column
                    int j = l5;
                    for (int i = 1; i <= kk1; ++i) {
                        ++j;
                        const double piv = h[i];
                        if (piv == 0.0) continue;
                        givens(piv, A1_(j, 1), cs, sn, sing);
                        int j1 = j;
                        for (int j2 = 1; j2 <= kDim; ++j2) { rota(cs, sn, xi[j2], Z_(j1)); j1 += n; }
                        if (i == kk1) break;
                        int i2 = 1;
                        for (int i1 = i + 1; i1 <= kk1; ++i1) { ++i2; rota(cs, sn, h[i1], A1_(j, i2)); }
                    }
                    for (int j2 = 1; j2 <= kDim; ++j2) fp = fp + xi[j2] * xi[j2];
                    continue;
                }
                if (jper == 0) {
                    for (int i = 1; i <= n7; ++i)
                        for (int j = 1; j <= kk; ++j) A2_(i, j) = 0.0;
                    int jk = n10 + 1;
                    for (int i = 1; i <= kk; ++i) {
                        int ik = jk;
                        for (int j = 1; j <= kk1; ++j) {
                            if (ik <= 0) break;
                            A2_(ik, i) = A1_(ik, j);
                            --ik;
                        }
                        ++jk;
                    }
                    jper = 1;
                }
                for (int i = 1; i <= kk; ++i) { h1[i] = 0.0; h2[i] = 0.0; }
                h1[kk1] = 0.0;
                {
                    int j = l5 - n10;
                    for (int i = 1; i <= kk1; ++i) {
                        ++j;
                        int l0 = j;
                        for (;;) {
                            const int l1 = l0 - kk;
                            if (l1 <= 0) { h2[l0] = h2[l0] + h[i]; break; }
                            if (l1 <= n10) { h1[l1] = h[i]; break; }
                            l0 = l1 - n10;
                        }
                    }
                }
                for (int j = 1; j <= n10; ++j) {
                    const double piv = h1[1];
                    if (piv == 0.0) {
                        for (int i = 1; i <= kk; ++i) h1[i] = h1[i + 1];
                        h1[kk1] = 0.0;
                        continue;
                    }
                    givens(piv, A1_(j, 1), cs, sn, sing);
                    int j1 = j;
                    for (int j2 = 1; j2 <= kDim; ++j2) { rota(cs, sn, xi[j2], Z_(j1)); j1 += n; }
                    for (int i = 1; i <= kk; ++i) rota(cs, sn, h2[i], A2_(j, i));
                    if (j == n10) break;
                    const int i2 = n10 - j < kk ? n10 - j : kk;
                    int i1 = 1;
                    for (int i = 1; i <= i2; ++i) {
                        i1 = i + 1;
                        rota(cs, sn, h1[i1], A1_(j, i1));
                        h1[i] = h1[i1];
                    }
                    h1[i1] = 0.0;
                }
                for (int j = 1; j <= kk; ++j) {
                    const int ij = n10 + j;
                    if (ij <= 0) continue;
                    const double piv = h2[j];
                    if (piv == 0.0) continue;
                    givens(piv, A2_(ij, j), cs, sn, sing);
                    int j1 = ij;
                    for (int j2 = 1; j2 <= kDim; ++j2) { rota(cs, sn, xi[j2], Z_(j1)); j1 += n; }
                    if (j == kk) break;
                    for (int i = j + 1; i <= kk; ++i) rota(cs, sn, h2[i], A2_(ij, i));
                }
                for (int j2 = 1; j2 <= kDim; ++j2) fp = fp + xi[j2] * xi[j2];
            }
            FP_(n) = fp0;
            FP_(n - 1) = fpold;
            NR_(n) = nplus;
            {
                int j1 = 0;
                for (int d = 0; d < kDim; ++d) {
                    back_periodic(a1, k1, a2, k, z + j1, n7, kk, c + j1, sing);
                    j1 += n;
                }
                for (int i = 1; i <= k; ++i) {
                    j1 = i;
                    for (int d = 0; d < kDim; ++d) { C_(j1 + n7) = C_(j1); j1 += n; }
                }
            }
            if (sing) return kUnchangedNonFinite;
            fpms = fp - s;
            n_out = n; fp_out = fp;
            if (std::fabs(fpms) < acc) return kFitted;
            if (fpms < 0.0) { part2 = true; break; }
            if (n == nmax) return kInterpolated;
            if (n == nest) return kIterationLimit;
            int npl1 = nplus * 2;
            const double rn = (double)nplus;
            if (fpold - fp > acc) {
                const double v = dv(rn * fpms, fpold - fp, sing);
                npl1 = (int)(v < 1073741824.0 ? v : 1073741824.0);
            }
            {
                int hi = npl1 > nplus / 2 ? npl1 : nplus / 2;
                if (hi < 1) hi = 1;
                nplus = nplus * 2 < hi ? nplus * 2 : hi;
            }
            fpold = fp;
            // residual of every knot interval, a data point on a knot shared half and half
            double fpart = 0.0;
            int i = 1, nw = 0;
            l = k1;
            jj = 0;
            for (int it = 1; it <= m1; ++it) {
                if (!(U_(it) < T_(l))) { nw = 1; ++l; }
                double term = 0.0;
                int l0 = l - k2;
                for (int d = 0; d < kDim; ++d) {
                    double fac = 0.0;
                    int j1 = l0;
                    for (int j = 1; j <= k1; ++j) { ++j1; fac = fac + C_(j1) * Q_(it, j); }
                    ++jj;
                    const double df = 1.0 * (fac - X_(jj));
                    term = term + df * df;
                    l0 += n;
                }
                fpart = fpart + term;
                if (nw == 0) continue;
                if (l > k2) {
                    const double store = term * 0.5;
                    FP_(i) = fpart - store;
                    ++i;
                    fpart = store;
                } else {
                    FP_(nrint) = term;
                }
                nw = 0;
            }
            FP_(nrint) = FP_(nrint) + fpart;
            for (int lk = 1; lk <= nplus; ++lk) {
                // split the knot interval with the largest residual at its middle data point
                const int kq = (n - nrint - 1) / 2;
                double fpmax = 0.0;
                int jbegin = 1, number = 0, maxpt = 0, maxbeg = 0;
                for (int j = 1; j <= nrint; ++j) {
                    const int jpoint = NR_(j);
                    if (!(fpmax >= FP_(j) || jpoint == 0)) { fpmax = FP_(j); number = j; maxpt = jpoint; maxbeg = jbegin; }
                    jbegin = jbegin + jpoint + 1;
                }
                if (number == 0) return kUnchangedNonFinite;        // no interval can take a knot (NaN residuals)
                const int ihalf = maxpt / 2 + 1, nrx = maxbeg + ihalf, nxt = number + 1;
                if (nxt <= nrint) {
                    for (int j = nxt; j <= nrint; ++j) {
                        const int j3 = nxt + nrint - j;
                        FP_(j3 + 1) = FP_(j3);
                        NR_(j3 + 1) = NR_(j3);
                        const int jk = j3 + kq;
                        T_(jk + 1) = T_(jk);
                    }
                }
                NR_(number) = ihalf - 1;
                NR_(nxt) = maxpt - ihalf;
                const double am = (double)maxpt;
                double an = (double)NR_(number);
                FP_(number) = dv(fpmax * an, am, sing);
                an = (double)NR_(nxt);
                FP_(nxt) = dv(fpmax * an, am, sing);
                T_(nxt + kq) = U_(nrx);
                ++n;
                ++nrint;
                if (n == nmax) { restart = true; break; }
                if (n == nest) break;
            }
            if (restart) break;
        }
        if (!part2 && !restart) return kIterationLimit;      // m trials without an acceptable knot set
        if (restart && interpolation_knots()) { n_out = n; fp_out = 0.0; return kInterpolated; }
    }

    // ---- the smoothing curve: F(p) = s ------------------------------------------------------------------------------
    {
        const int nk1 = n - k1, nrint = nk1 - k;
        const double fac = dv((double)nrint, T_(nk1 + 1) - T_(k1), sing);
        double hd[2 * kMaxDegree + 4];
        for (int l = k2; l <= nk1; ++l) {
            const int lmk = l - k1;
            for (int j = 1; j <= k1; ++j) {
                const int ik = j + k1, lj = l + j, lk = lj - k2;
                hd[j] = T_(l) - T_(lk);
                hd[ik] = T_(l) - T_(lj);
            }
            int lp = lmk;
            for (int j = 1; j <= k2; ++j) {
                int jk = j;
                double prod = hd[j];
                for (int i = 1; i <= k; ++i) { ++jk; prod = prod * hd[jk] * fac; }
                const int lk = lp + k1;
                BB_(lmk, j) = dv(T_(lk) - T_(lp), prod, sing);
                ++lp;
            }
        }
    }
    double p1 = 0.0, f1 = fp0 - s, p3 = -1.0, f3 = fpms;
    const int n11 = n10 - 1, n8 = n7 - 1;
    double p = 0.0;
    {
        int l = n7;
        bool border_only = false;
        for (int i = 1; i <= k; ++i) {
            const int j = k + 1 - i;
            p = p + A2_(l, j);
            --l;
            if (l == 0) { border_only = true; break; }
        }
        if (!border_only)
            for (int i = 1; i <= n10; ++i) p = p + A1_(i, 1);
    }
    p = dv((double)n7, p, sing);
    int ich1 = 0, ich3 = 0;
    const int nc = kDim * n;
    for (int itp = 1; itp <= kMaxIter; ++itp) {
        if (sing) return kUnchangedNonFinite;
        const double pinv = dv(1.0, p, sing);
        double cs, sn;
        for (int i = 1; i <= nc; ++i) C_(i) = Z_(i);
        for (int i = 1; i <= n7; ++i) {
            G1_(i, k1) = A1_(i, k1);
            G1_(i, k2) = 0.0;
            G2_(i, 1) = 0.0;
            for (int j = 1; j <= k; ++j) { G1_(i, j) = A1_(i, j); G2_(i, j + 1) = A2_(i, j); }
        }
        {
            int l = n10;
            for (int j = 1; j <= k1; ++j) {
                if (l <= 0) break;
                G2_(l, 1) = A1_(l, j);
                --l;
            }
        }
        for (int it = 1; it <= n8; ++it) {
            if (sing) return kUnchangedNonFinite;
            for (int j = 1; j <= kDim; ++j) xi[j] = 0.0;
            for (int i = 1; i <= k1; ++i) { h1[i] = 0.0; h2[i] = 0.0; }
            h1[k2] = 0.0;
            int l;
            bool rotate_band;
            if (it <= n11) {
                l = it;
                int l0 = it, j = 1;
                while (j <= k2) {
                    if (l0 == n10) {
                        l0 = 1;
                        for (int l1 = j; l1 <= k2; ++l1) { h2[l0] = BB_(it, l1) * pinv; ++l0; }
                        break;
                    }
                    h1[j] = BB_(it, j) * pinv;
                    ++l0;
                    ++j;
                }
                rotate_band = true;
            } else {
                l = 1;
                int i = it - n10;
                for (int j = 1; j <= k2; ++j) {
                    ++i;
                    int l0 = i;
                    for (;;) {
                        const int l1 = l0 - k1;
                        if (l1 <= 0) { h2[l0] = h2[l0] + BB_(it, j) * pinv; break; }
                        if (l1 <= n11) { h1[l1] = BB_(it, j) * pinv; break; }
                        l0 = l1 - n11;
                    }
                }
                rotate_band = n11 > 0;
            }
            if (rotate_band) {
                for (int j = l; j <= n11; ++j) {
                    const double piv = h1[1];
                    givens(piv, G1_(j, 1), cs, sn, sing);
                    int j1 = j;
                    for (int j2 = 1; j2 <= kDim; ++j2) { rota(cs, sn, xi[j2], C_(j1)); j1 += n; }
                    for (int i = 1; i <= k1; ++i) rota(cs, sn, h2[i], G2_(j, i));
                    if (j == n11) break;
                    const int i2 = n11 - j < k1 ? n11 - j : k1;
                    int i1 = 1;
                    for (int i = 1; i <= i2; ++i) {
                        i1 = i + 1;
                        rota(cs, sn, h1[i1], G1_(j, i1));
                        h1[i] = h1[i1];
                    }
                    h1[i1] = 0.0;
                }
            }
            for (int j = 1; j <= k1; ++j) {
                const int ij = n11 + j;
                if (ij <= 0) continue;
                const double piv = h2[j];
                givens(piv, G2_(ij, j), cs, sn, sing);
                int j1 = ij;
                for (int j2 = 1; j2 <= kDim; ++j2) { rota(cs, sn, xi[j2], C_(j1)); j1 += n; }
                if (j == k1) break;
                for (int i = j + 1; i <= k1; ++i) rota(cs, sn, h2[i], G2_(ij, i));
            }
        }
        {
            int j1 = 0;
            for (int d = 0; d < kDim; ++d) {
                back_periodic(g1, k2, g2, k1, c + j1, n7, k1, c + j1, sing);
                j1 += n;
            }
            for (int i = 1; i <= k; ++i) {
                j1 = i;
                for (int d = 0; d < kDim; ++d) { C_(j1 + n7) = C_(j1); j1 += n; }
            }
        }
        fp = 0.0;
        {
            int l = k1, jj = 0;
            for (int it = 1; it <= m1; ++it) {
                if (!(U_(it) < T_(l))) ++l;
                int l0 = l - k2;
                double term = 0.0;
                for (int d = 0; d < kDim; ++d) {
                    double fac = 0.0;
                    int j1 = l0;
                    for (int j = 1; j <= k1; ++j) { ++j1; fac = fac + C_(j1) * Q_(it, j); }
                    ++jj;
                    const double df = fac - X_(jj);
                    term = term + df * df;
                    l0 += n;
                }
                fp = fp + term * (1.0 * 1.0);
            }
        }
        if (sing) return kUnchangedNonFinite;
        fpms = fp - s;
        n_out = n; fp_out = fp;
        if (std::fabs(fpms) < acc) return kFitted;
        if (itp == kMaxIter) return kIterationLimit;
        const double p2 = p, f2 = fpms;
        if (ich3 == 0) {
            if (!((f2 - f3) > acc)) {
                p3 = p2; f3 = f2;
                p = p * 0.04;
                if (p <= p1) p = p1 * 0.9 + p2 * 0.1;
                continue;
            }
            if (f2 < 0.0) ich3 = 1;
        }
        if (ich1 == 0) {
            if (!((f1 - f2) > acc)) {
                p1 = p2; f1 = f2;
                p = dv(p, 0.04, sing);
                if (p3 < 0.0) continue;
                if (p >= p3) p = p2 * 0.1 + p3 * 0.9;
                continue;
            }
            if (f2 > 0.0) ich1 = 1;
        }
        if (f2 >= f1 || f2 <= f3) return kIterationLimit;
        if (p3 > 0.0) {
            const double r1 = f1 * (f2 - f3), r2 = f2 * (f3 - f1), r3 = f3 * (f1 - f2);
            p = dv(-(p1 * p2 * r3 + p2 * p3 * r1 + p3 * p1 * r2), p1 * r1 + p2 * r2 + p3 * r3, sing);
        } else {
            p = dv(p1 * (f1 - f3) * f2 - p2 * (f2 - f3) * f1, (f1 - f2) * f3, sing);
        }
        if (f2 < 0.0) { p3 = p2; f3 = f2; }
        else          { p1 = p2; f1 = f2; }
    }
    return kIterationLimit;
#undef X_
#undef Z_
#undef C_
#undef FP_
#undef NR_
#undef A1_
#undef A2_
#undef BB_
#undef G1_
#undef G2_
#undef Q_
}

// point i of the m evaluation points u = i * (1 / m) on the curve (t, c, n knots, degree k); false if singular
MM_HD bool evaluate(const double* t, const double* c, int n, int k, int m, int i, double out[3])
{
    const int k1 = k + 1, nk1 = n - k1;
    const double arg = (double)i * (1.0 / (double)m);
    int l = k1, sing = 0;
    while (!(arg < T_(l + 1) || l == nk1)) ++l;
    double h[kMaxDegree + 4];
    bspl(t, k, arg, l, h, sing);
    for (int d = 0; d < kDim; ++d) {
        double sp = 0.0;
        int ll = l - k1 + d * n;
        for (int j = 1; j <= k1; ++j) { ++ll; sp = sp + c[ll - 1] * h[j]; }
        out[d] = sp;
    }
    return sing == 0;
}

#undef T_
#undef U_

}  // namespace bspl
}  // namespace mm
