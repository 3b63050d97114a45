"""The culled matrix-pipe screen's tile bound (csrc/mm_tile_bound.h), checked on the host against f64.

k_screen_mx_cull skips a 32 x 32 tile when its threshold thr(I, J) is at least the current row and column minima of the
tile; the screened value of a candidate stays bit-identical only if thr never exceeds a squared distance the screen can
compute for the tile, i.e. thr <= (exact squared distance) - e2 for every point pair of the tile.  mm_tile_bound_probe runs
the kernel's own f32 code on the host; here every tile pair of adversarial sets is compared with the f64 distances of the
rotated points -- exactly rotated by the f32 (cos, sin), and rotated the way the kernel does it (two f32 fma) -- and every
point is checked to lie inside its tile's circle."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

U = 2.0 ** -24


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    import multimoda_rs_amd as mm
    return mm._native


def _f32_fma(a, b, c):
    """f32 fma(a, b, c) for f32 inputs: the f64 product of two f32 values is exact, the sum rounds once in f64 (far below
    the slack checked here) and once to f32."""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(np.float32)


def _probe(native, ref, tgt, e, c, s, e2):
    rx, ry = (np.ascontiguousarray(ref[:, k], dtype=np.float32) for k in (0, 1))
    tx, ty = (np.ascontiguousarray(tgt[:, k], dtype=np.float32) for k in (0, 1))
    nrt, nct = (len(rx) + 31) // 32, (len(tx) + 31) // 32
    circ = np.zeros(4 * (nrt + nct), dtype=np.float32)
    thr = np.zeros(nrt * nct, dtype=np.float32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = native.lib().mm_tile_bound_probe(P(rx), P(ry), len(rx), P(tx), P(ty), len(tx), int(e), C.c_float(c), C.c_float(s),
                                          float(e2), P(circ), P(thr))
    assert rc == 0, native.last_error()
    return (rx, ry, tx, ty), circ.reshape(-1, 4), thr.reshape(nrt, nct)


def _check(native, ref, tgt, angles):
    """ref, tgt: f64 point sets around the rotation centre (0, 0); every threshold against the f64 distances."""
    ref32, tgt32 = ref.astype(np.float32), tgt.astype(np.float32)
    ra = np.hypot(ref32[:, 0].astype(np.float64), ref32[:, 1].astype(np.float64)).max()
    rb = np.hypot(tgt32[:, 0].astype(np.float64), tgt32[:, 1].astype(np.float64)).max()
    rmax = max(ra, rb)
    e = 9 - int(np.frexp(rmax * (1.0 + 1e-6))[1])                     # the engine's scale exponent: radius in [256, 512)
    R = ra + rb
    e2 = U * (47 * R * R + 6 * ra * ra + 27 * rb * rb)                   # mx_e2 (csrc/mm_level_plan.cpp)
    S = np.float32(2.0 ** e)
    skipped = 0
    for ang in angles:
        c, s = np.float32(np.cos(ang)), np.float32(np.sin(ang))
        (rx, ry, tx, ty), circ, thr = _probe(native, ref32, tgt32, e, c, s, e2)
        nrt, nct = thr.shape
        ax, ay = (S * rx).astype(np.float64), (S * ry).astype(np.float64)
        bx, by = S * tx, S * ty                                          # f32, as the kernel holds them
        # the rotated target: exactly (f64) by the f32 cos / sin, and as the kernel rounds it
        ex = bx.astype(np.float64) * np.float64(c) - by.astype(np.float64) * np.float64(s)
        ey = bx.astype(np.float64) * np.float64(s) + by.astype(np.float64) * np.float64(c)
        kx = _f32_fma(bx, c, -(by * s)).astype(np.float64)
        ky = _f32_fma(bx, s, by * c).astype(np.float64)
        e2s = e2 * 2.0 ** (2 * e)
        # every point inside its circle (rows unrotated; columns: the unrotated circle rotated exactly contains the exact
        # rotation of its points)
        for i in range(nrt):
            idx = np.minimum(np.arange(32 * i, 32 * i + 32), len(rx) - 1)
            assert (np.hypot(ax[idx] - circ[i, 0], ay[idx] - circ[i, 1]) <= circ[i, 2]).all()
        for i in range(nrt):
            ri = np.minimum(np.arange(32 * i, 32 * i + 32), len(rx) - 1)
            for j in range(nct):
                if not thr[i, j] > 0:
                    continue
                skipped += 1
                cj = np.minimum(np.arange(32 * j, 32 * j + 32), len(tx) - 1)
                d2e = (ax[ri, None] - ex[None, cj]) ** 2 + (ay[ri, None] - ey[None, cj]) ** 2
                d2k = (ax[ri, None] - kx[None, cj]) ** 2 + (ay[ri, None] - ky[None, cj]) ** 2
                low = min(d2e.min(), d2k.min()) - e2s
                assert float(thr[i, j]) <= low, (ang, i, j, float(thr[i, j]), low)
    return skipped


def _contour(rng, n, r, cx=0.0, cy=0.0, wobble=0.1):
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    rr = r * (1 + wobble * np.sin(3 * t + rng.uniform(0, 6)))
    return np.stack([cx + rr * np.cos(t), cy + rr * np.sin(t)], axis=1)


ANGLES = np.concatenate([np.linspace(-np.pi, np.pi, 13)[:-1], [0.0, 1e-7, np.pi / 2, 0.7853981633974483]])


def test_contours_are_culled_and_the_bound_holds(native):
    rng = np.random.default_rng(3)
    a = _contour(rng, 521, 2.0)
    b = _contour(rng, 521, 2.1)
    assert _check(native, a, b, ANGLES) > 1000            # most tile pairs of two contours have a threshold


@pytest.mark.parametrize("scale", [1.0, 2.0 ** -7, 3.0e4, 1e-20, 1e20])
def test_adversarial_sets(native, scale):
    rng = np.random.default_rng(11)
    cases = []
    # a far outlier that fixes the scale; everything else tiny
    small = rng.normal(0, 2.0 ** -9, (96, 2))
    far = small.copy(); far[0] = (500.0, -100.0)
    cases += [(far, small + 2.0 ** -11), (small + 2.0 ** -11, far)]
    # collinear points, duplicates
    line = np.stack([np.linspace(-400, 400, 223), np.zeros(223)], axis=1)
    cases += [(line, line[::-1].copy()), (line, line + (0.0, 3.0))]
    dup = np.repeat(rng.uniform(-300, 300, (8, 2)), 16, axis=0)
    cases += [(dup, dup.copy()), (dup, _contour(rng, 96, 350.0))]
    # radii just below the 512 edge of the scale, and just above 256
    for rmax in (511.99, 256.01):
        p = _contour(rng, 544, rmax / 1.1)
        q = _contour(rng, 65, rmax / 1.1)
        cases += [(p, q), (q, p)]
    # coordinates on f16 ties at the top of the scale
    t = np.sort(rng.uniform(0, 2 * np.pi, 64))
    tie = np.stack([511.875 * np.cos(t), 511.875 * np.sin(t)], axis=1)
    tie = (np.floor(tie / 0.25) + 0.5) * 0.25
    cases += [(tie, tie * 0.5)]
    for ref, tgt in cases:
        _check(native, ref * scale, tgt * scale, ANGLES[:6])


def test_no_threshold_for_touching_circles(native):
    rng = np.random.default_rng(5)
    a = _contour(rng, 128, 100.0, wobble=0.0)
    _, _, thr = _probe(native, a.astype(np.float32), a.astype(np.float32), -6, np.float32(1.0), np.float32(0.0), 0.0)
    assert not (np.diag(thr) > 0).any()                 # a tile against itself
