"""The culled screen's split layout on the device (k_screen_mx_cull with PairDesc::ref_main / tgt_main): a set of two runs,
lumen ++ catheter, gets tiles per run wherever that adds no tile (csrc/mm_tile_bound.h, mm_engine_set_screen_split), at the
smallest shapes where the slot -> point mapping can go wrong.  Every case asserts:
  * the values of the full kernel, of the culled kernel without split and of the culled kernel with split are BIT-identical;
  * `total` (the tiles the full kernel computes) is unchanged;
  * `done` lies in the [lo, hi] bracket of the two-phase rule (tests/test_gpu_screen_cull_dispatch.py, whose construction
    is copied here) computed from the split probe (mm_tile_bound_probe_split) and the slot map (mm_tile_slot_map) of the
    layout the engine's condition takes.

The issue's case "40 + 20" cannot reach the kernel: the matrix-pipe screen takes sets of 64 .. 544 points, and 60 points
are screened exactly.  That its split is refused is pinned on the host (tests/test_tile_split_host.py); here the case runs
at 44 + 20, the smallest set with a 20-point catheter that the screen takes and whose split would add a tile (64 points:
2 tiles, split 2 + 1)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24


def _scale(ref, tgt):
    r32, t32 = ref.astype(np.float32).astype(np.float64), tgt.astype(np.float32).astype(np.float64)
    ra, rb = np.hypot(r32[:, 0], r32[:, 1]).max(), np.hypot(t32[:, 0], t32[:, 1]).max()
    e = 9 - int(np.frexp(max(ra, rb) * (1.0 + 1e-6))[1])
    R = ra + rb
    return e, U * (47 * R * R + 6 * ra * ra + 27 * rb * rb)


def _slots(mm, n, main):
    """(slot -> point of the layout the engine takes for (n, main), the main it takes)."""
    L = mm._native.lib()
    take = L.mm_tile_slot_map(int(n), int(main), 0, None)
    assert take >= 0
    out = np.zeros(32 * ((n + 31) // 32), dtype=np.int32)
    assert L.mm_tile_slot_map(int(n), int(take), len(out), out.ctypes.data_as(C.c_void_p)) == take
    return out, take


def _thr(mm, ref, tgt, mains, angle, e, e2):
    """thr[nrt, nct] of one candidate for the layout `mains`, by the kernel's own f32 code run on the host."""
    rx, ry = (np.ascontiguousarray(ref[:, k], dtype=np.float32) for k in (0, 1))
    tx, ty = (np.ascontiguousarray(tgt[:, k], dtype=np.float32) for k in (0, 1))
    nrt, nct = (len(rx) + 31) // 32, (len(tx) + 31) // 32
    circ = np.zeros(4 * (nrt + nct), dtype=np.float32)
    thr = np.zeros(nrt * nct, dtype=np.float32)
    P = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = mm._native.lib().mm_tile_bound_probe_split(P(rx), P(ry), len(rx), P(tx), P(ty), len(tx), int(mains[0]), int(mains[1]),
                                                    int(e), C.c_float(np.cos(angle)), C.c_float(np.sin(angle)), float(e2),
                                                    P(circ), P(thr))
    assert rc == 0
    return thr.reshape(nrt, nct)


def _phase1(thr):
    close = ~(thr > 0)
    m1 = close.copy()
    for i in np.nonzero(~close.any(axis=1))[0]:
        m1[i, np.argmin(thr[i])] = True
    for j in np.nonzero(~close.any(axis=0))[0]:
        m1[np.argmin(thr[:, j]), j] = True
    return m1


def _tile_bounds(mm, ref, tgt, split, angles, e, e2):
    """(lower, upper) count of the tiles the two-phase rule computes over all candidates, for the layout the engine takes
    when asked for `split` (tests/test_gpu_screen_cull_dispatch.py: the phase-1 minima replaced by f64 squared distances
    -/+ the screen's error bound)."""
    S = 2.0 ** e
    a = S * ref.astype(np.float32).astype(np.float64)
    b0 = S * tgt.astype(np.float32).astype(np.float64)
    e2s = e2 * S * S * (1 + 2.0 ** -17)
    nrt, nct = (len(a) + 31) // 32, (len(b0) + 31) // 32
    ri, rm = _slots(mm, len(a), split[0])
    ci, cm = _slots(mm, len(b0), split[1])
    lo = hi = 0
    for ang in angles:
        c, s = np.float64(np.float32(np.cos(ang))), np.float64(np.float32(np.sin(ang)))
        b = np.stack([b0[:, 0] * c - b0[:, 1] * s, b0[:, 0] * s + b0[:, 1] * c], axis=1)
        d2 = ((a[ri, None, :] - b[None, ci, :]) ** 2).sum(axis=2)
        thr = _thr(mm, ref, tgt, (rm, cm), ang, e, e2).astype(np.float64)
        m1 = _phase1(thr)
        big = np.where(np.repeat(np.repeat(m1, 32, axis=0), 32, axis=1), d2, np.inf)
        u = big.min(axis=1).reshape(nrt, 32).max(axis=1)
        v = big.min(axis=0).reshape(nct, 32).max(axis=1)
        n1 = int(m1.sum())
        lo += n1 + int((~m1 & (thr < np.maximum(u[:, None], v[None, :]) - e2s)).sum())
        hi += n1 + int((~m1 & ~(thr > np.maximum(u[:, None], v[None, :]) + e2s)).sum())
    return lo, hi, (rm, cm)


def _run(engine, ref, tgt, angles, **kw):
    t0 = engine.screen_tiles()
    v, e2 = engine.screen_values(ref, tgt, angles, (0.0, 0.0), **kw)
    t1 = engine.screen_tiles()
    return v, e2, t1[0] - t0[0], t1[1] - t0[1]


def _same(engine, mm, ref, tgt, split, angles):
    """The three kernels' values, the tile counts and their brackets; returns (done unsplit, done split, mains taken)."""
    full, e2a, _, _ = _run(engine, ref, tgt, angles, cull=False, split=split)
    plain, e2b, done0, total0 = _run(engine, ref, tgt, angles, cull=True)
    cut, e2c, done1, total1 = _run(engine, ref, tgt, angles, cull=True, split=split)
    assert e2a == e2b == e2c
    for other in (plain, cut):
        bad = np.nonzero(full.view(np.uint32) != other.view(np.uint32))[0]
        assert bad.size == 0, (bad[:8], full[bad[:8]], other[bad[:8]])
    assert total0 == total1 == len(angles) * ((len(ref) + 31) // 32) * ((len(tgt) + 31) // 32)
    e, _ = _scale(ref, tgt)
    lo0, hi0, _ = _tile_bounds(mm, ref, tgt, (0, 0), angles, e, e2a)
    lo1, hi1, mains = _tile_bounds(mm, ref, tgt, split, angles, e, e2a)
    print("tiles of %d: unsplit %d in [%d, %d], split %s -> taken %s: %d in [%d, %d]" %
          (total0, done0, lo0, hi0, split, mains, done1, lo1, hi1))
    assert 0 < done0 <= total0 and lo0 <= done0 <= hi0, (done0, lo0, hi0)
    assert 0 < done1 <= total1 and lo1 <= done1 <= hi1, (done1, lo1, hi1)
    return done0, done1, mains


def _lumen(n, r=2.3, phase=0.0, squash=0.8):
    """A wobbling ring around the rotation centre."""
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    rr = r * (1 + 0.08 * np.sin(3 * t + phase) + 0.04 * np.cos(5 * t - phase))
    return np.stack([rr * np.cos(t), squash * rr * np.sin(t)], axis=1)


def _catheter(n, at=(0.1, -0.05)):
    """A small central ring (radius 0.5)."""
    u = np.linspace(0, 2 * np.pi, n, endpoint=False) + 0.3
    return np.stack([at[0] + 0.5 * np.cos(u), at[1] + 0.5 * np.sin(u)], axis=1)


def _set(lum, cath, r=2.3, phase=0.0, at=(0.1, -0.05)):
    return np.concatenate([_lumen(lum, r, phase), _catheter(cath, at)])


A61 = np.radians(np.linspace(-180.0, 180.0, 61))


def test_split_both_sides_3x3(engine, mm):
    """53 + 20 on both sides: 3 x 3 tiles (the chain variant), lumen padding and catheter padding on either side.  (On a
    closed contour of two tiles every tile is close to every other: all 9 are computed in either layout, the case checks
    the values.)"""
    ref, tgt = _set(53, 20), _set(53, 20, r=2.35, phase=0.7, at=(-0.05, 0.1))
    _, _, mains = _same(engine, mm, ref, tgt, (53, 53), A61)
    assert mains == (53, 53)


@pytest.mark.parametrize("lum,cath", [(64, 20), (53, 32)])
def test_runs_that_end_on_a_tile_edge(engine, mm, lum, cath):
    """64 + 20: the lumen ends on a tile edge (no lumen padding).  53 + 32: the catheter fills its tile exactly."""
    ref, tgt = _set(lum, cath), _set(lum, cath, r=2.35, phase=0.7, at=(-0.05, 0.1))
    _, _, mains = _same(engine, mm, ref, tgt, (lum, lum), A61)
    assert mains == (lum, lum)


@pytest.mark.parametrize("lum,cath", [(44, 20), (53, 40), (85, 40), (90, 70), (60, 36)])
def test_split_that_adds_a_tile_is_refused(engine, mm, lum, cath):
    """44 + 20 (64 points: 2 tiles, split 2 + 1; module docstring for 40 + 20), 53 + 40 (3 -> 2 + 2), 85 + 40 (4 -> 3 + 2),
    90 + 70 (5 -> 3 + 3), 60 + 36 (3 -> 2 + 2): the engine keeps the consecutive layout, `done` is the same with and
    without the request."""
    ref, tgt = _set(lum, cath), _set(lum, cath, r=2.35, phase=0.7, at=(-0.05, 0.1))
    done0, done1, mains = _same(engine, mm, ref, tgt, (lum, lum), A61)
    assert mains == (0, 0)
    assert done0 == done1


def test_two_tile_catheter_that_qualifies(engine, mm):
    """A catheter run longer than one tile qualifies when the remainders of the two runs sum past 32: 60 + 37 (97 points:
    4 tiles, split 2 + 2) is the smallest with a 60-point lumen; the catheter's second tile holds 5 points and padding."""
    ref, tgt = _set(60, 37), _set(60, 37, r=2.35, phase=0.7, at=(-0.05, 0.1))
    _, _, mains = _same(engine, mm, ref, tgt, (60, 60), A61)
    assert mains == (60, 60)


@pytest.mark.parametrize("side", [0, 1])
def test_one_side_split(engine, mm, side):
    """One side 53 + 20, the other a plain 96-point contour, both ways round."""
    cut, plain = _set(53, 20), _lumen(96, r=2.35, phase=0.7)
    ref, tgt = (cut, plain) if side == 0 else (plain, cut)
    split = (53, 0) if side == 0 else (0, 53)
    _, _, mains = _same(engine, mm, ref, tgt, split, A61)
    assert mains == split


def _model_ratio(ref, tgt, angles):
    """done(split) / done(consecutive) of tools/model_cull_tiles.py for these inputs."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import model_cull_tiles as model
    p1, p2 = model.count_tiles(ref, tgt, angles)
    q1, q2 = model.count_tiles(ref, tgt, angles, model.split_main(len(ref), 501), model.split_main(len(tgt), 501))
    return (q1.sum() + q2.sum()) / (p1.sum() + p2.sum())


def test_17_column_tiles_against_3_row_tiles(engine, mm):
    """The set-bit variant: target 501 + 20 (17 column tiles) against reference 53 + 20 (3 row tiles), 5 rotations."""
    ref, tgt = _set(53, 20), _set(501, 20, r=2.35, phase=0.7, at=(-0.05, 0.1))
    _, _, mains = _same(engine, mm, ref, tgt, (53, 501), np.radians(np.linspace(-30.0, 30.0, 5)))
    assert mains == (53, 501)


def test_17_x_17_tiles_computes_fewer(engine, mm):
    """501 + 20 against 501 + 20 at 0, 90 and 179.5 degrees: the split layout computes fewer than 0.9 of the tiles.  The
    model (tools/model_cull_tiles.py) gives 0.80 as the mean of four frame pairs of the flagship workload over 91
    rotations; the margin to 0.9 covers the spread from pair to pair and angle to angle, and the model's ratio for these
    very inputs is asserted below the same 0.9."""
    ref, tgt = _set(501, 20), _set(501, 20, r=2.35, phase=0.7, at=(-0.05, 0.1))
    angles = np.radians([0.0, 90.0, 179.5])
    done0, done1, mains = _same(engine, mm, ref, tgt, (501, 501), angles)
    assert mains == (501, 501)
    ratio = _model_ratio(ref, tgt, angles)
    print("done split / unsplit: device %.3f, model %.3f" % (done1 / done0, ratio))
    assert ratio < 0.9
    assert done1 < 0.9 * done0, (done1, done0)


def test_within_plan_switch(engine, mm):
    """WithinPlan on the benchmark's `tiny` workload (4 pullbacks x 12 frames x 501 + 20 points, 181 rotations): the logs
    with the switch on and off are identical, fewer tiles are computed with it on, and a resident plan keeps the switch it
    was staged with."""
    def run(create_on, run_on):
        case = mm.synthetic_case(12, 501)
        engine.set_screen_split(create_on)
        try:
            plan = mm.WithinPlan(engine, case, 2.0, 180.0, True, 501, precision=mm.MM_PRECISION_F32_MATRIX)
            engine.set_screen_split(run_on)
            t0 = engine.screen_tiles()
            logs, evals, unresolved = plan.run()
            t1 = engine.screen_tiles()
            plan.close()
        finally:
            engine.set_screen_split(True)
        return logs, evals, unresolved, t1[0] - t0[0], t1[1] - t0[1], [g.lumen.copy() for g in case]

    on, off, kept = run(True, True), run(False, False), run(True, False)
    assert on[:3] == off[:3] == kept[:3]
    for a, b, c in zip(on[5], off[5], kept[5]):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert on[4] == off[4] == kept[4] > 0
    print("tiny: tiles done with the split %d, without %d, of %d" % (on[3], off[3], on[4]))
    assert 0 < on[3] < off[3] <= off[4]
    assert kept[3] == on[3]
