"""The culled screen's group followers that leave after phase 1 (k_screen_mx_cull at 17 column tiles, WorkItem::pad = 8): a
follower whose met row minima stay at or below Tr_I and whose met column minima stay at or below Tc_J (the smallest thr of
the row tile / column tile outside the followers' phase 1) has empty phase-2 masks, and exactly then; it skips the column
maxima, the masks and phase 2.  Every case asserts, for a forced G = 8:
  * the screened values are BIT-identical to the full kernel's and to the culled kernel's with G = 1;
  * `done` (the tiles computed) lies in the bracket of the group rule (tests/test_gpu_screen_cull_group.py);
  * mm_engine_screen_early's followers are the followers the reported work items imply;
  * its early exits lie in [lo, hi]: lo the followers whose phase-2 mask is empty for certain, hi those whose mask is not
    non-empty for certain.

The bracket of the early exits follows the tile bracket's convention: thr of the group from the kernel's own f32 code
(mm_tile_bound_probe_group), phase-1 minima as f64 squared distances taken at -/+ the screen's error bound e2, and the two
hand-over masks C_lo <= carry <= C_hi of the leader.  With p_lo = m1 | C_lo and p_hi = m1 | C_hi,
    a follower leaves for certain when   ~p_lo & ~(thr > maxima(p_lo) + e2)   is empty (its real mask lies inside it),
    and stays for certain when           ~p_hi &  (thr < maxima(p_hi) - e2)   is not (that one lies inside its real mask).
Each case first asserts ON THE CPU, before anything runs on the device, that it certainly holds the followers it is there
for: some that leave and some that stay, only ones that leave, or only ones that stay."""
import numpy as np
import pytest

from test_gpu_screen_cull_group import (REF3, TGT17, _flagship_pairs, _group_bounds, _phase1, _run, _scale, _set, _slots,
                                        _thr_group)

pytestmark = pytest.mark.gpu

G = 8


def _items(n):
    """The work items a forced G = 8 gives a list of n <= 32 candidates: one item (a forced size asks for items of four
    groups), a list of one has no group."""
    assert 1 <= n <= 4 * G
    return [(0, n, G if n > 1 else 1)]


def _followers(items):
    return sum(min(g0 + g, a0 + cnt) - g0 - 1 for a0, cnt, g in items for g0 in range(a0, a0 + cnt, g))


def _early_bounds(mm, ref, tgt, split, angles, items):
    """(followers, those that certainly leave after phase 1, those that certainly stay) over the work items."""
    e, e2 = _scale(ref, tgt)
    S = 2.0 ** e
    a = S * ref.astype(np.float32).astype(np.float64)
    b0 = S * tgt.astype(np.float32).astype(np.float64)
    e2s = e2 * S * S * (1 + 2.0 ** -17)
    nrt, nct = (len(a) + 31) // 32, (len(b0) + 31) // 32
    ri, rm = _slots(mm, len(a), split[0])
    ci, cm = _slots(mm, len(b0), split[1])

    def maxima(d2, mask):
        big = np.where(np.repeat(np.repeat(mask, 32, axis=0), 32, axis=1), d2, np.inf)
        u = big.min(axis=1).reshape(nrt, 32).max(axis=1)
        v = big.min(axis=0).reshape(nct, 32).max(axis=1)
        return np.maximum(u[:, None], v[None, :])

    fol = leave = stay = 0
    for a0, cnt, g in items:
        for g0 in range(a0, a0 + cnt, g):
            grp = angles[g0:min(g0 + g, a0 + cnt)]
            thr = _thr_group(mm, ref, tgt, (rm, cm), grp, e, e2)
            m1 = _phase1(thr)
            c_lo = c_hi = np.zeros_like(m1)
            for k, ang in enumerate(grp):
                c, s = np.float64(np.float32(np.cos(ang))), np.float64(np.float32(np.sin(ang)))
                b = np.stack([b0[:, 0] * c - b0[:, 1] * s, b0[:, 0] * s + b0[:, 1] * c], axis=1)
                d2 = ((a[ri, None, :] - b[None, ci, :]) ** 2).sum(axis=2)
                p_lo, p_hi = m1 | c_lo, m1 | c_hi
                sure = ~p_hi & (thr < maxima(d2, p_hi) - e2s)
                upper = ~p_lo & ~(thr > maxima(d2, p_lo) + e2s)
                if k == 0:
                    # the leader's hand-over, as the tile bracket takes it (p_lo == p_hi == m1 here)
                    c_lo, c_hi = sure, upper
                else:
                    fol += 1
                    leave += not upper.any()
                    stay += bool(sure.any())
    return fol, leave, stay


def _case(engine, mm, ref, tgt, split, angles, expect):
    """CPU: the case holds what `expect` names ("both", "leave", "stay", None).  Device: values, tiles, counters.
    Returns (followers, early exits)."""
    angles = np.ascontiguousarray(angles, dtype=np.float64)
    items = _items(len(angles))
    fol, leave, stay = _early_bounds(mm, ref, tgt, split, angles, items)
    print("followers %d: certainly leave after phase 1 %d, certainly stay %d" % (fol, leave, stay))
    assert fol == _followers(items) and leave + stay <= fol
    if expect == "both":
        assert leave > 0 and stay > 0, (fol, leave, stay)
    elif expect == "leave":
        assert fol > 0 and leave == fol, (fol, leave, stay)
    elif expect == "stay":
        assert fol > 0 and stay == fol, (fol, leave, stay)
    lo, hi = leave, fol - stay

    full, e2a, _, _, _ = _run(engine, ref, tgt, angles, split, None, cull=False)
    y0 = engine.screen_early()
    one, e2b, _, total, _ = _run(engine, ref, tgt, angles, split, None)
    y1 = engine.screen_early()
    v, e2g, done, tot, got = _run(engine, ref, tgt, angles, split, G)
    y2 = engine.screen_early()
    assert e2a == e2b == e2g and tot == total
    for name, w in (("G = 1", one), ("G = 8", v)):
        bad = np.nonzero(full.view(np.uint32) != w.view(np.uint32))[0]
        assert bad.size == 0, (name, bad[:8], full[bad[:8]], w[bad[:8]])
    assert got.tolist() == [list(i) for i in items], got
    t_lo, t_hi = _group_bounds(mm, ref, tgt, split, angles, items)
    early, followers = y2[0] - y1[0], y2[1] - y1[1]
    print("tiles done %d of %d, the group rule's count in [%d, %d]; followers %d, left after phase 1 %d, bracket [%d, %d]" %
          (done, tot, t_lo, t_hi, followers, early, lo, hi))
    assert y1 == y0, "G = 1 has no followers"
    assert 0 < done <= tot and t_lo <= done <= t_hi, (done, t_lo, t_hi)
    assert followers == fol
    assert lo <= early <= hi, (early, lo, hi)
    return followers, early


@pytest.mark.parametrize("pair", [1, 2, 3, 4])
def test_flagship_pairs(engine, mm, pair):
    """Frame pairs 1 - 4 of synthetic_pullback(12, 501), three runs of eight rotations 0.5 degrees apart (the inputs of
    test_cost_cap_on_the_flagship_shape): 21 followers each, some that leave and some that stay."""
    _, pairs = _flagship_pairs()
    (ref, rm), (tgt, tm) = pairs[pair - 1]
    angles = np.radians(np.concatenate([s + 0.5 * np.arange(8) for s in (-180.0, -60.5, 33.0)]))
    fol, _ = _case(engine, mm, ref, tgt, (rm, tm), angles, "both")
    assert fol == 21


def test_three_row_tiles(engine, mm):
    """3 x 17 tiles, nine rotations 0.5 degrees apart: a group of eight (followers of both kinds) and a lone leader."""
    fol, _ = _case(engine, mm, REF3, TGT17, (53, 501), np.radians(-4.0 + 0.5 * np.arange(9)), "both")
    assert fol == 7


SET17 = _set(501, 20)


def test_every_follower_leaves(engine, mm):
    """17 x 17 tiles, nine rotations 0.5 degrees apart: every follower leaves after phase 1."""
    fol, early = _case(engine, mm, SET17, TGT17, (501, 501), np.radians(-4.0 + 0.5 * np.arange(9)), "leave")
    assert early == fol == 7


def test_every_follower_stays(engine, mm):
    """The same sets, 18 rotations 20 degrees apart: the leader's tiles are not the followers', every one falls back to
    the general path."""
    fol, early = _case(engine, mm, SET17, TGT17, (501, 501), np.radians(-170.0 + 20.0 * np.arange(18)), "stay")
    assert fol == 15 and early == 0


def test_mixed_followers(engine, mm):
    """The same sets, 16 rotations 2 degrees apart: followers of both kinds in each group."""
    fol, _ = _case(engine, mm, SET17, TGT17, (501, 501), np.radians(-16.0 + 2.0 * np.arange(16)), "both")
    assert fol == 14


@pytest.mark.parametrize("n_angles, followers", [(1, 0), (7, 6)])
def test_lone_leader_and_partial_group(engine, mm, n_angles, followers):
    """A list of one (no group, no follower) and a partial group of seven (six followers)."""
    fol, early = _case(engine, mm, REF3, TGT17, (53, 501), np.radians(-4.0 + 0.5 * np.arange(n_angles)), None)
    assert fol == followers and early <= fol


def test_switch_off_counts_nothing(engine, mm):
    """WithinPlan on the benchmark's `tiny` workload with the group switch off: no followers, no early exits; the counter
    does not move (forced to 2 it does)."""
    def run(group):
        case = mm.synthetic_case(12, 501)
        engine.set_screen_group(group)
        try:
            plan = mm.WithinPlan(engine, case, 2.0, 180.0, True, 501, precision=mm.MM_PRECISION_F32_MATRIX)
            y0 = engine.screen_early()
            out = plan.run()
            y1 = engine.screen_early()
            plan.close()
        finally:
            engine.set_screen_group(0)
        return out, y0, y1

    off, y0, y1 = run(1)
    assert y1 == y0, (y0, y1)
    two, z0, z1 = run(2)
    assert two == off
    assert z1[1] > z0[1] and 0 <= z1[0] - z0[0] <= z1[1] - z0[1], (z0, z1)
