// mm_winding_device.h -- the arithmetic of "winding number" (include/mm_ccta.h) as C++ for host and device: the half solid
// angle of a face as a complex number (Van Oosterom-Strackee), the quarter-turn bookkeeping that keeps a running angle
// without atan2, the per-face flags, and the fold of two partial angles.  Every operation is unfused f64 in the order
// written (the files that include it are built with -ffp-contract=off); frexp and ldexp are exact.  So the kernel
// (mm_winding_kernels.hip), the host hook (mm_winding.cpp) and the checker (tests/mm_checkers/winding_number.py) produce
// the same bits.  Internal.
#pragma once

#include <cstdint>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MM_WIND_HD __host__ __device__ __forceinline__
#else
#define MM_WIND_HD inline
#endif

namespace mm {
namespace winding {

constexpr int kChunk = 256;        // staged faces a chunk: 256 x 9 doubles = 18 KiB of LDS
constexpr int kMaxGroups = 16;     // partial records a query
constexpr int kQpt = 2;            // queries a lane
constexpr double kTouch = 0x1p-47;     // touch: den <= 0 and |num| <= kTouch * L
constexpr double kTinyZ = 0x1p-600;    // zero face: max(|den|, |num|) below this ...
constexpr double kTinyLen2 = 0x1p-960; // ... or a squared corner distance below this (0 included)

// A running angle n * pi/2 + arg(pr + i pi), pr >= |pi|, with the flags folded so far.  32 bytes: the partial record.
struct State {
    double pr, pi, rho;
    int32_t n, touch;
};
static_assert(sizeof(State) == 32, "a partial record is 32 bytes");

MM_WIND_HD State start()
{
    return State{1.0, 0.0, __builtin_inf(), 0, 0};
}

// rotate (re, im) into the cone re >= |im| by an exact multiple of 90 degrees; returns the multiple taken out
MM_WIND_HD int cone(double& re, double& im)
{
    const double r = re, i = im;
    if (i > r && i >= -r && i > 0.0) { re = i; im = -r; return 1; }
    if (i < -r && i <= r && i < 0.0) { re = -i; im = r; return -1; }
    if (r < 0.0) { re = -r; im = -i; return i >= 0.0 ? 2 : -2; }
    return 0;
}

// s += m quarter turns + arg(zr + i zi), (zr, zi) in the cone
MM_WIND_HD void turn(State& s, int m, double zr, double zi)
{
    double qr = s.pr * zr - s.pi * zi, qi = s.pr * zi + s.pi * zr;
    const int m2 = cone(qr, qi);
    s.n += m + m2;
    int e;
    (void)__builtin_frexp(qr, &e);
    s.pr = __builtin_ldexp(qr, -e);
    s.pi = __builtin_ldexp(qi, -e);
}

// one face (A, B, C) seen from p
MM_WIND_HD void face(State& s, double px, double py, double pz, double Ax, double Ay, double Az, double Bx, double By,
                     double Bz, double Cx, double Cy, double Cz)
{
    const double ax = Ax - px, ay = Ay - py, az = Az - pz;
    const double bx = Bx - px, by = By - py, bz = Bz - pz;
    const double cx = Cx - px, cy = Cy - py, cz = Cz - pz;
    const double aa = (ax * ax + ay * ay) + az * az, bb = (bx * bx + by * by) + bz * bz, cc = (cx * cx + cy * cy) + cz * cz;
    const double la = __builtin_sqrt(aa), lb = __builtin_sqrt(bb), lc = __builtin_sqrt(cc);
    const double L = (la * lb) * lc;
    const double ux = by * cz - bz * cy, uy = bz * cx - bx * cz, uz = bx * cy - by * cx;
    const double num = (ax * ux + ay * uy) + az * uz;
    const double ab = (ax * bx + ay * by) + az * bz, bc = (bx * cx + by * cy) + bz * cz, ca = (cx * ax + cy * ay) + cz * az;
    const double den = ((la * lb) * lc + ab * lc) + (bc * la + ca * lb);
    const double an = __builtin_fabs(num), ad = __builtin_fabs(den);
    const double mx = ad > an ? ad : an;
    double least = aa < bb ? aa : bb;
    least = cc < least ? cc : least;
    if (mx < kTinyZ || least < kTinyLen2) {   // the zero face: not folded
        s.rho = 0.0;
        return;
    }
    if (den <= 0.0 && an <= kTouch * L) s.touch = 1;
    const double rho = mx / L;
    s.rho = rho < s.rho ? rho : s.rho;
    double zr = den, zi = num;
    const int m = cone(zr, zi);
    turn(s, m, zr, zi);
}

// s += t: two partial angles
MM_WIND_HD void join(State& s, const State& t)
{
    s.touch |= t.touch;
    s.rho = t.rho < s.rho ? t.rho : s.rho;
    turn(s, t.n, t.pr, t.pi);
}

}  // namespace winding
}  // namespace mm
