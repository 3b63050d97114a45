"""The culled screen's value floor on the device (k_screen_mx_cull at 17 column tiles, ScreenOptions::screen_floor,
mm_screen_values_floor): a candidate's value is the MAXIMUM of its minima, so after phase 1 only the rows and columns whose
minimum lies above the largest minimum that is already exact (the floor L) get phase-2 tiles.  Every case asserts

  * the screened values with the floor on are BIT-identical to those with it off and to the full kernel's;
  * `done` (the tiles computed) and the followers that left after phase 1 lie in the bracket of the rule restated in numpy.

The bracket follows tests/test_gpu_screen_cull_group.py / _early.py: thr of a group from the kernel's own f32 code on the host
(mm_tile_bound_probe_group), minima as f64 squared distances taken at -/+ the screen's error bound e2, and the two hand-over
masks C_lo <= carry <= C_hi of the leader, p_lo = m1 | C_lo, p_hi = m1 | C_hi.  With u_lo / u_hi the minima over p_hi less e2
and over p_lo plus e2 (a larger mask only lowers a minimum) and Tr_lo / Tr_hi the smallest thr outside p_lo / p_hi:
    a row is settled for certain if u_hi <= Tr_lo, and perhaps if u_lo <= Tr_hi;
    L_lo = the largest u_lo of the rows and columns settled for certain, L_hi = the largest u_hi of those settled perhaps;
    a row is live for certain if u_lo > L_hi, and perhaps unless u_hi <= L_lo;
    the tiles computed for certain: p_lo and every other tile with thr < the largest u_lo of its certainly live rows /
    columns; perhaps: p_hi and every other tile whose thr is not above the largest u_hi of its perhaps live ones.
A follower leaves for certain if nothing of it is perhaps live, and stays for certain if something is live for certain.
Each case first asserts ON THE CPU that the two ends of its brackets are a few tiles apart at the most."""
import numpy as np
import pytest

import cull_floor_cases as cf
from test_gpu_screen_cull_group import _flagship_pairs, _phase1, _scale, _slots, _thr_group

pytestmark = pytest.mark.gpu

NONE = -np.inf
SPLIT3, SPLIT17 = (76, 501), (501, 501)


def _bounds(mm, ref, tgt, split, angles, items, floor):
    """(tiles lo, tiles hi, followers, followers that leave for certain, that stay for certain) over the work items."""
    e, e2 = _scale(ref, tgt)
    S = 2.0 ** e
    a = S * ref.astype(np.float32).astype(np.float64)
    b0 = S * tgt.astype(np.float32).astype(np.float64)
    e2s = e2 * S * S * (1 + 2.0 ** -17)
    nrt, nct = (len(a) + 31) // 32, (len(b0) + 31) // 32
    ri, rm = _slots(mm, len(a), split[0])
    ci, cm = _slots(mm, len(b0), split[1])

    def minima(d2, mask):
        big = np.where(cf.tile_mask(mask), d2, np.inf)
        return big.min(axis=1), big.min(axis=0)

    def outside(thr, mask):
        o = np.where(mask, np.inf, thr)
        return np.repeat(o.min(axis=1), 32), np.repeat(o.min(axis=0), 32)

    def tile_max(x, keep, n):
        return np.where(keep, x, NONE).reshape(n, 32).max(axis=1)

    t_lo = t_hi = fol = leave = stay = 0
    for a0, cnt, G in items:
        for g0 in range(a0, a0 + cnt, G):
            grp = angles[g0:min(g0 + G, a0 + cnt)]
            thr = _thr_group(mm, ref, tgt, (rm, cm), grp, e, e2)
            m1 = _phase1(thr)
            c_lo = c_hi = np.zeros_like(m1)
            for k, ang in enumerate(grp):
                c, s = np.float64(np.float32(np.cos(ang))), np.float64(np.float32(np.sin(ang)))
                b = np.stack([b0[:, 0] * c - b0[:, 1] * s, b0[:, 0] * s + b0[:, 1] * c], axis=1)
                d2 = ((a[ri, None, :] - b[None, ci, :]) ** 2).sum(axis=2)
                p_lo, p_hi = m1 | c_lo, m1 | c_hi
                (ru, cu), (rl, cl) = minima(d2, p_lo), minima(d2, p_hi)
                u_hi, v_hi, u_lo, v_lo = ru + e2s, cu + e2s, rl - e2s, cl - e2s
                if floor:
                    (tr_lo, tc_lo), (tr_hi, tc_hi) = outside(thr, p_lo), outside(thr, p_hi)
                    L_lo = max(0.0, u_lo[u_hi <= tr_lo].max(initial=0.0), v_lo[v_hi <= tc_lo].max(initial=0.0))
                    L_hi = max(0.0, u_hi[u_lo <= tr_hi].max(initial=0.0), v_hi[v_lo <= tc_hi].max(initial=0.0))
                    live_r, live_c = u_lo > L_hi, v_lo > L_hi               # for certain
                    may_r, may_c = ~(u_hi <= L_lo), ~(v_hi <= L_lo)          # perhaps
                else:
                    live_r = may_r = np.ones(nrt * 32, dtype=bool)
                    live_c = may_c = np.ones(nct * 32, dtype=bool)
                w_lo = np.maximum(tile_max(u_lo, live_r, nrt)[:, None], tile_max(v_lo, live_c, nct)[None, :])
                w_hi = np.maximum(tile_max(u_hi, may_r, nrt)[:, None], tile_max(v_hi, may_c, nct)[None, :])
                sure = ~p_lo & (thr < w_lo)
                maybe = ~p_hi & ~(thr > w_hi)
                t_lo += int(p_lo.sum()) + int(sure.sum())
                t_hi += int(p_hi.sum()) + int(maybe.sum())
                if k == 0:
                    c_lo, c_hi = sure, maybe
                else:
                    # a follower leaves exactly when its phase-2 masks are empty (the kernel's header)
                    fol += 1
                    leave += not (~p_lo & ~(thr > w_hi)).any()
                    stay += bool((~p_hi & (thr < w_lo)).any())
    return t_lo, t_hi, fol, leave, stay


def _screen(engine, ref, tgt, split, angles, group, floor, pair=True, cull=True):
    engine.set_screen_pair(pair)
    try:
        t0, y0 = engine.screen_tiles(), engine.screen_early()
        v, _, items = engine.screen_values_floor(ref, tgt, angles, (0.0, 0.0), group, floor, cull=cull, split=split)
        t1, y1 = engine.screen_tiles(), engine.screen_early()
    finally:
        engine.set_screen_pair(True)
    return v, t1[0] - t0[0], (y1[0] - y0[0], y1[1] - y0[1]), items


def _case(engine, mm, ref, tgt, split, angles, group, pair=True, width=None):
    """Floor on against off against the full kernel; both runs inside their brackets.  Returns (tiles off, tiles on,
    early off, early on).  width: the most the ends of a bracket may be apart (default: two tiles a candidate)."""
    angles = np.ascontiguousarray(angles, dtype=np.float64)
    full, _, _, _ = _screen(engine, ref, tgt, split, angles, group, False, pair, cull=False)
    off, t_off, y_off, items = _screen(engine, ref, tgt, split, angles, group, False, pair)
    on, t_on, y_on, items_on = _screen(engine, ref, tgt, split, angles, group, True, pair)
    assert np.array_equal(items, items_on)
    for name, w in (("floor off", off), ("floor on", on)):
        bad = np.nonzero(full.view(np.uint32) != w.view(np.uint32))[0]
        assert bad.size == 0, (name, bad[:8], full[bad[:8]], w[bad[:8]])
    width = 2 * len(angles) if width is None else width
    for name, floor, t, y in (("off", False, t_off, y_off), ("on", True, t_on, y_on)):
        lo, hi, fol, leave, stay = _bounds(mm, ref, tgt, split, angles, items.tolist(), floor)
        print("G = %d, pair %d, floor %s: tiles %d in [%d, %d]; followers %d, left after phase 1 %d in [%d, %d]" %
              (group, pair, name, t, lo, hi, y[1], y[0], leave, fol - stay))
        assert hi - lo <= width and leave + stay <= fol, (lo, hi, fol, leave, stay)
        assert lo <= t <= hi, (name, t, lo, hi)
        assert y[1] == fol and leave <= y[0] <= fol - stay, (name, y, fol, leave, stay)
    assert t_on <= t_off
    return t_off, t_on, y_off[0], y_on[0]


@pytest.mark.parametrize("group, n_angles, pair", [(1, 9, True), (2, 9, True), (4, 7, True), (4, 7, False), (4, 10, True),
                                                   (8, 9, True), (8, 10, True), (8, 10, False), (8, 23, True), (8, 23, False),
                                                   (8, 64, True)])
def test_contour_three_row_tiles(engine, mm, group, n_angles, pair):
    """521 target points against 96 (17 x 3 tiles), rotations 0.5 degrees apart: full groups, a partial group (7 at G = 4, 23
    at G = 8), a lone leader (9) and a lone follower (10: a group of two behind full groups) -- a pair's X without its Y;
    64: several work items.  Pairs on and off where a group has pairs."""
    _case(engine, mm, cf.REF3, cf.TGT17, SPLIT3, np.radians(-4.0 + 0.5 * np.arange(n_angles)), group, pair)


@pytest.mark.parametrize("group", [1, 2, 4, 8])
def test_contour_saves_tiles(engine, mm, group):
    """521 against 521 points (17 x 17 tiles), 17 rotations 0.5 degrees apart: strictly fewer tiles with the floor.  (The
    followers that leave after phase 1 may be fewer or more: the leader hands fewer tiles on, a follower's phase 1 is
    smaller; the brackets say which.)"""
    t_off, t_on, _, _ = _case(engine, mm, cf.SET17, cf.TGT17, SPLIT17, np.radians(-4.0 + 0.5 * np.arange(17)), group)
    assert t_on < t_off, (t_on, t_off)


def test_flagship_pairs_against_the_model(engine, mm):
    """Frame pairs 1 - 4 of synthetic_pullback(12, 501), three runs of eight rotations 0.5 degrees apart at G = 8: the device's
    tiles with the floor against tools/model_cull_tiles.py --floor (exact minima there: a few tiles apart), and strictly
    fewer than with the floor off."""
    model, pairs = _flagship_pairs()
    angles = np.radians(np.concatenate([s + 0.5 * np.arange(8) for s in (-180.0, -60.5, 33.0)]))
    dev_on = dev_off = mod_on = 0
    for (ref, rm), (tgt, tm) in pairs:
        t_off, t_on, _, _ = _case(engine, mm, ref, tgt, (rm, tm), angles, 8)
        p1, p2 = model.count_tiles(ref, tgt, angles, model.split_main(len(ref), rm), model.split_main(len(tgt), tm), 8, True, True)
        dev_on += t_on; dev_off += t_off; mod_on += int(p1.sum() + p2.sum())
    n = 4 * len(angles)
    print("tiles per candidate: device floor off %.1f, floor on %.1f, model with the floor %.1f" % (dev_off / n, dev_on / n, mod_on / n))
    assert dev_on < dev_off
    assert abs(dev_on - mod_on) <= 0.02 * mod_on, (dev_on, mod_on)


def _directed(engine, mm, case, claim):
    """A directed case of tests/test_cull_floor_rule.py: its claim shown on the CPU (with the model's thresholds, for the
    group sizes the device then runs), then on the device at G = 1 and G = 8."""
    ref, tgt, mains, angles = case
    assert len(tgt) == 521 and len(ref) in (96, 521)
    for group in (1, 8):
        assert claim(cf.screen(ref, tgt, angles, group, True, True, mains)), group
        _case(engine, mm, ref, tgt, mains, angles, group)


def test_a_live_row_made_exact_in_phase_2_is_the_value(engine, mm):
    """(a)"""
    def claim(cs):
        return any(c.fu.max() == c.value > c.fv.max() and c.u[np.argmax(c.fu)] > c.L and not c.srow[np.argmax(c.fu)] and
                   c.fu.max() < c.u[np.argmax(c.fu)] for c in cs)
    _directed(engine, mm, cf.case_outlier(), claim)


def test_the_floor_comes_from_a_column(engine, mm):
    """(b)"""
    _directed(engine, mm, cf.case_column_floor(),
              lambda cs: any(c.L > 0 and c.v[c.scol].max(initial=0.0) == c.L > c.u[c.srow].max(initial=0.0) for c in cs))


def test_nothing_settled(engine, mm):
    """(c) L = 0"""
    _directed(engine, mm, cf.case_nothing_settled(), lambda cs: any(not c.srow.any() and not c.scol.any() and c.L == 0.0 for c in cs))


def test_ties(engine, mm):
    """(e) minima equal to the floor, in rows and columns that are not settled.  The screened values of an orbit agree only
    as far as the matrix pipe's products do, so the brackets, not the ties, are what the device is held to here."""
    def claim(cs):
        c = cs[0]
        return c.L > 0 and ((c.u == c.L) & ~c.srow).any() and ((c.v == c.L) & ~c.scol).any()
    ref, tgt, mains, angles = cf.case_ties()
    _directed(engine, mm, (ref, tgt, mains, angles), claim)


def test_far_rotations(engine, mm):
    """(f) 18 rotations 20 degrees apart in groups of eight, against 96 points (the CPU test's case) and against 521, where
    followers stay: a pair then runs the general path twice, X's floor and then Y's.  Pairs on and off."""
    ref, tgt, mains, angles = cf.case_far_group()
    for pair in (True, False):
        _case(engine, mm, ref, tgt, mains, angles, 8, pair)
        _, _, _, early = _case(engine, mm, cf.SET17, tgt, SPLIT17, angles, 8, pair)
        assert early < 15


def test_stale_scratch(engine, mm):
    """A three-row-tile case behind a different 17-row-tile case on the same engine (row stores, thr table and column
    maxima hold the other pair's 17 row tiles): the values and counters of a fresh engine."""
    _case(engine, mm, cf.SET17, cf.TGT17, SPLIT17, np.radians(-16.0 + 2.0 * np.arange(16)), 8)
    angles = np.radians(-4.0 + 0.5 * np.arange(10))
    v, t, y, _ = _screen(engine, cf.REF3, cf.TGT17, SPLIT3, angles, 8, True)
    with mm.Engine() as fresh:
        w, t_f, y_f, _ = _screen(fresh, cf.REF3, cf.TGT17, SPLIT3, angles, 8, True)
    assert np.array_equal(v.view(np.uint32), w.view(np.uint32))
    assert t == t_f and y == y_f, (t, t_f, y, y_f)


def test_within_plan_switch(engine, mm):
    """WithinPlan on the benchmark's `tiny` workload with the switch on, off and on again: logs, evals, unresolved and moved
    coordinates are identical, fewer tiles with the switch on, and the setter round-trips (on again: the first run's tiles)."""
    def run(on):
        case = mm.synthetic_case(12, 501)
        engine.set_screen_floor(on)
        try:
            plan = mm.WithinPlan(engine, case, 2.0, 180.0, True, 501, precision=mm.MM_PRECISION_F32_MATRIX)
            t0 = engine.screen_tiles()
            logs, evals, unresolved = plan.run()
            t1 = engine.screen_tiles()
            plan.close()
        finally:
            engine.set_screen_floor(True)
        return logs, evals, unresolved, t1[0] - t0[0], t1[1] - t0[1], [g.lumen.copy() for g in case]

    on, off, again = run(True), run(False), run(True)
    assert on[:3] == off[:3] == again[:3]
    for a, b, c in zip(on[5], off[5], again[5]):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    print("tiny: tiles done with the floor %d, without %d, of %d" % (on[3], off[3], on[4]))
    assert on[4] == off[4] == again[4] > 0
    assert 0 < on[3] < off[3] <= off[4]
    assert again[3] == on[3]
    assert mm._native.lib().mm_engine_set_screen_floor(None, 1) != 0
