"""The culled screen's tile loop (k_screen_mx_cull at 17 column tiles visits the SET bits of a row tile's mask, the column
tile reached by a wave-uniform register index; below 17 it keeps the bit-test chain: the *_17 cases repeat the small shapes'
properties on targets of 544 points) and its per-candidate bookkeeping (thr by a 2-D lane layout, masks by ballot, a column's nearest
row tile found in the same sweep) on the smallest shapes at which they can go wrong.  Every case: the culled values are
BIT-identical to the full kernel's and 0 < done <= total.

Tiles done.  The masks follow from thr(I, J) (mm_tile_bound_probe, the kernel's own f32 operations on the host) and, in
phase 2, from the row and column minima after phase 1, which the host does not have bit for bit.  So:
  * where every thr <= 0 (the concentric circles) phase 1 takes every tile: done == total, exactly;
  * elsewhere done lies between two counts of the two-phase rule restated in numpy with the phase-1 minima replaced by
    f64 squared distances -/+ the screen's error bound e2 (a screened value is within e2 of the exact one): a tile outside
    the upper count was provably skippable, a tile inside the lower count provably not.  The device's square root may differ
    from the host's by an ulp, which can move a thr across 0 or across a minimum only when they agree to that ulp: the
    sets here are generic, the counts are asserted as they stand.
"""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _scale(ref, tgt):
    """The engine's scale exponent and error bound for sets around the rotation centre (0, 0) (tests/test_tile_bound_host.py)."""
    r32, t32 = ref.astype(np.float32).astype(np.float64), tgt.astype(np.float32).astype(np.float64)
    ra, rb = np.hypot(r32[:, 0], r32[:, 1]).max(), np.hypot(t32[:, 0], t32[:, 1]).max()
    e = 9 - int(np.frexp(max(ra, rb) * (1.0 + 1e-6))[1])
    R = ra + rb
    return e, U * (47 * R * R + 6 * ra * ra + 27 * rb * rb)


def _thr(mm, ref, tgt, angle, e, e2):
    """thr[nrt, nct] of one candidate, by the kernel's own f32 code run on the host."""
    rx, ry = (np.ascontiguousarray(ref[:, k], dtype=np.float32) for k in (0, 1))
    tx, ty = (np.ascontiguousarray(tgt[:, k], dtype=np.float32) for k in (0, 1))
    nrt, nct = (len(rx) + 31) // 32, (len(tx) + 31) // 32
    circ = np.zeros(4 * (nrt + nct), dtype=np.float32)
    thr = np.zeros(nrt * nct, dtype=np.float32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = mm._native.lib().mm_tile_bound_probe(P(rx), P(ry), len(rx), P(tx), P(ty), len(tx), int(e), C.c_float(np.cos(angle)),
                                              C.c_float(np.sin(angle)), float(e2), P(circ), P(thr))
    assert rc == 0
    return thr.reshape(nrt, nct)


def _phase1(thr):
    """The phase-1 masks of the kernel header: every tile with thr <= 0; a row tile without one takes its smallest thr
    (lowest column on a tie); then a column tile without a close tile takes its nearest row tile (lowest row on a tie)."""
    close = ~(thr > 0)
    m1 = close.copy()
    for i in np.nonzero(~close.any(axis=1))[0]:
        m1[i, np.argmin(thr[i])] = True
    for j in np.nonzero(~close.any(axis=0))[0]:
        m1[np.argmin(thr[:, j]), j] = True
    return m1


def _tile_bounds(mm, ref, tgt, angles, e, e2):
    """(lower, upper) count of the tiles the two-phase rule computes over all candidates (module docstring)."""
    S = 2.0 ** e
    a = S * ref.astype(np.float32).astype(np.float64)
    b0 = S * tgt.astype(np.float32).astype(np.float64)
    e2s = e2 * S * S * (1 + 2.0 ** -17)
    nrt, nct = (len(a) + 31) // 32, (len(b0) + 31) // 32
    ri = np.minimum(np.arange(nrt * 32), len(a) - 1)
    ci = np.minimum(np.arange(nct * 32), len(b0) - 1)
    lo = hi = 0
    for ang in angles:
        c, s = np.float64(np.float32(np.cos(ang))), np.float64(np.float32(np.sin(ang)))
        b = np.stack([b0[:, 0] * c - b0[:, 1] * s, b0[:, 0] * s + b0[:, 1] * c], axis=1)
        d2 = ((a[ri, None, :] - b[None, ci, :]) ** 2).sum(axis=2)
        thr = _thr(mm, ref, tgt, ang, e, e2).astype(np.float64)
        m1 = _phase1(thr)
        big = np.where(np.repeat(np.repeat(m1, 32, axis=0), 32, axis=1), d2, np.inf)
        u = big.min(axis=1).reshape(nrt, 32).max(axis=1)               # Umax_I, exact
        v = big.min(axis=0).reshape(nct, 32).max(axis=1)               # Vmax_J, exact
        n1 = int(m1.sum())
        lo += n1 + int((~m1 & (thr < np.maximum(u[:, None], v[None, :]) - e2s)).sum())
        hi += n1 + int((~m1 & ~(thr > np.maximum(u[:, None], v[None, :]) + e2s)).sum())
    return lo, hi


def _same(engine, mm, ref, tgt, angles, count=True):
    full, e2a = engine.screen_values(ref, tgt, angles, (0.0, 0.0), cull=False)
    t0 = engine.screen_tiles()
    cull, e2b = engine.screen_values(ref, tgt, angles, (0.0, 0.0), cull=True)
    t1 = engine.screen_tiles()
    assert e2a == e2b
    bad = np.nonzero(full.view(np.uint32) != cull.view(np.uint32))[0]
    assert bad.size == 0, (bad[:8], full[bad[:8]], cull[bad[:8]])
    done, total = t1[0] - t0[0], t1[1] - t0[1]
    assert total == len(angles) * ((len(ref) + 31) // 32) * ((len(tgt) + 31) // 32)
    assert 0 < done <= total
    if count:
        e, _ = _scale(ref, tgt)
        lo, hi = _tile_bounds(mm, ref, tgt, angles, e, e2a)
        print("tiles done %d of %d, the rule's count in [%d, %d]" % (done, total, lo, hi))
        assert lo <= done <= hi, (done, lo, hi)
    return done, total


def _circle(n, r, phase=0.0):
    t = phase + np.linspace(0, 2 * np.pi, n, endpoint=False)
    return np.stack([r * np.cos(t), r * np.sin(t)], axis=1)


def _ellipse(n, a=8.0, b=1.0):
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    return np.stack([a * np.cos(t), b * np.sin(t)], axis=1)


def _ring(n):
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    r = 3.0 * (1 + 0.15 * np.sin(3 * t))
    return np.stack([r * np.cos(t), r * np.sin(t)], axis=1)


@pytest.mark.parametrize("n", [64, 96])
def test_every_bit_set(engine, mm, n):
    """2 x 2 and 3 x 3 tiles, every mask full: the set-bit loop runs to the last tile, an even and an odd count."""
    ref, tgt = _circle(n, 5.0), _circle(n, 5.0, phase=0.01)
    angles = np.radians(np.linspace(-180.0, 180.0, 61))
    e, e2 = _scale(ref, tgt)
    for ang in angles:
        assert not (_thr(mm, ref, tgt, ang, e, e2) > 0).any()
    done, total = _same(engine, mm, ref, tgt, angles, count=False)
    assert done == total


def test_one_bit_per_row_tile(engine, mm):
    """An elongated contour (an ellipse of axis ratio 8, 160 points, 5 x 5 tiles) against itself scaled by 1.01, at 0 and
    +-1 degree; and against a target whose tile J is a cluster of 32 points at the middle of arc J.  On the closed contour
    consecutive arcs touch, so no row tile has exactly one close tile (thr <= 0) there -- counted on the host at all three
    angles -- and the one-tile path (the loop's prologue is its epilogue) is reached by the clustered target: the assertion below."""
    ref = _ellipse(160)
    angles = np.radians([0.0, 1.0, -1.0])
    _same(engine, mm, ref, ref * 1.01, angles)
    rng = np.random.default_rng(1)
    mid = ref.reshape(5, 32, 2)[:, 16, :] * 1.01
    tgt = (mid[:, None, :] + rng.normal(0, 0.02, (5, 32, 2))).reshape(160, 2)
    e, e2 = _scale(ref, tgt)
    for ang in angles:
        assert ((~(_thr(mm, ref, tgt, ang, e, e2) > 0)).sum(axis=1) == 1).any()    # a row tile with exactly one close tile
    _same(engine, mm, ref, tgt, angles)


def test_lone_column_tile(engine, mm):
    """A column tile without a close partner: it takes the tile of its nearest row tile.  The ellipse against a 96-point
    ellipse of half the size, shifted along the long axis until its far end leaves every arc of the reference."""
    ref = _ellipse(160)
    tgt = _ellipse(96) * 0.5 + (10.0, 0.0)
    angles = np.radians([0.0, 1.0, -1.0])
    e, e2 = _scale(ref, tgt)
    for ang in angles:
        thr = _thr(mm, ref, tgt, ang, e, e2)
        assert (thr > 0).all(axis=0).any() and (~(thr > 0)).any()      # a lone column tile, and close tiles besides
    _same(engine, mm, ref, tgt, angles)


@pytest.mark.parametrize("nr,nt", [(544, 544), (544, 64), (64, 544)])
def test_highest_and_lowest_tile_index(engine, mm, nr, nt):
    rng = np.random.default_rng(nr + nt)
    base = _ring(544)
    ref = base[:: 544 // nr][:nr] if nr < 544 else base
    tgt = base * 1.02 + rng.normal(0, 0.01, base.shape)
    tgt = tgt[:nt]
    ref = ref[:nr]
    _same(engine, mm, ref, tgt, np.radians(np.linspace(-30.0, 30.0, 5)))


@pytest.mark.parametrize("n_angles", [1, 2, 3, 5, 33])
def test_candidate_counts_not_divisible_by_four(engine, mm, n_angles):
    rng = np.random.default_rng(223)
    ref = _ring(223)
    tgt = ref * 1.02 + rng.normal(0, 0.01, ref.shape)
    _same(engine, mm, ref, tgt, np.radians(np.linspace(-30.0, 30.0, n_angles)))


# ---- the same properties at 17 column tiles (targets of 544 points), where the set-bit loop and the ballot masks run ----

def _clusters17(ref):
    """17 column tiles, each a cluster of 32 points: 15 along the reference ellipse (1.01 outside it), one far above arc 1
    and one far left of arc 2 -- two lone column tiles, the nearest row tile of one odd, of the other even."""
    rng = np.random.default_rng(17)
    t = np.linspace(0, 2 * np.pi, 15, endpoint=False) + 0.2
    mid = np.concatenate([1.01 * np.stack([8.0 * np.cos(t), np.sin(t)], axis=1), [(-2.0, 12.0), (-16.0, 0.0)]])
    return (mid[:, None, :] + rng.normal(0, 0.02, (17, 32, 2))).reshape(544, 2)


def test_one_bit_and_lone_columns_17(engine, mm):
    """5 row tiles: the two lone column tiles, the nearest row tile of one odd (the upper half of the wave wins the meet),
    of the other even.  17 row tiles: row tiles with exactly one close tile, and one with none (its nearest partner)."""
    ref, big = _ellipse(160), _ellipse(544)
    tgt = _clusters17(ref)
    angles = np.radians([0.0, 1.0, -1.0])
    e, e2 = _scale(ref, tgt)
    for ang in angles:
        thr = _thr(mm, ref, tgt, ang, e, e2)
        lone = np.nonzero((thr > 0).all(axis=0))[0]
        near = np.argmin(thr[:, lone], axis=0)
        assert (near % 2 == 1).any() and (near % 2 == 0).any()
        thr = _thr(mm, big, tgt, ang, e, e2)
        assert ((~(thr > 0)).sum(axis=1) == 1).any() and (thr > 0).all(axis=1).any() and (thr > 0).all(axis=0).any()
    _same(engine, mm, ref, tgt, angles)
    _same(engine, mm, big, tgt, angles)


def test_every_bit_set_17(engine, mm):
    """Everything but one far point (it fixes the scale) inside a tiny disc: every one of the 17 bits of every mask is set."""
    ref, tgt = _circle(64, 0.05), _circle(544, 0.05, phase=0.01)
    tgt[0] = (10.0, 0.0)
    angles = np.radians(np.linspace(-180.0, 180.0, 7))
    e, e2 = _scale(ref, tgt)
    for ang in angles:
        assert not (_thr(mm, ref, tgt, ang, e, e2) > 0).any()
    done, total = _same(engine, mm, ref, tgt, angles, count=False)
    assert done == total


@pytest.mark.parametrize("n_angles", [1, 2, 3, 5, 33])
def test_candidate_counts_not_divisible_by_four_17(engine, mm, n_angles):
    rng = np.random.default_rng(544)
    ref = _ring(544)[::3]
    tgt = _ring(544) * 1.02 + rng.normal(0, 0.01, (544, 2))
    _same(engine, mm, ref, tgt, np.radians(np.linspace(-30.0, 30.0, n_angles)))
