"""The culled screen's paired followers (k_screen_mx_cull at 17 column tiles, WorkItem::pad = G >= 4, mm_engine_set_screen_pair):
behind a group's leader the followers run their phase 1 two at a time -- one pass over the group's tile list, one tile index
and one A fragment for both, the second follower's row minima in a row store of its own -- and each then takes the followers'
exit test and, if it stays, the general path on its own registers.

The yardstick is never the paired path itself: the same build with the switch off (every follower alone, the path before
pairs) and the full kernel (set_screen_cull off).  Every case asserts
  * the screened values BIT-identical (the f32 bits) with the switch on, with it off, and against the full kernel;
  * mm_engine_screen_tiles' computed tiles and both words of mm_engine_screen_early equal, exactly, switch on against off.

Shapes: the 501 + 20 target (17 column tiles: the only variant with groups) against the 53 + 20 reference (three row tiles, the
last partly filled), closed contours in contour order as in tests/test_gpu_screen_cull_early.py::test_three_row_tiles, at
most 32 rotations a call; one run on frame pair 1 of synthetic_pullback(12, 501), 521 + 521 points in the split layout."""
import functools
import os
import sys

import numpy as np
import pytest

from test_gpu_screen_cull_group import REF3, TGT17, _flagship_pairs, _set

pytestmark = pytest.mark.gpu

SPLIT3 = (53, 501)


def _screen(engine, ref, tgt, split, angles, group, pair, cull=True):
    """(values, tiles computed, (followers that left early, followers)) of one call, the pair switch as given."""
    engine.set_screen_pair(pair)
    try:
        t0, y0 = engine.screen_tiles(), engine.screen_early()
        v, _, items = engine.screen_values_group(ref, tgt, angles, (0.0, 0.0), group, cull=cull, split=split)
        t1, y1 = engine.screen_tiles(), engine.screen_early()
    finally:
        engine.set_screen_pair(True)
    return v, t1[0] - t0[0], (y1[0] - y0[0], y1[1] - y0[1]), items


def _same(engine, ref, tgt, split, angles, group):
    """Switch on against switch off against the full kernel.  Returns (values, tiles, (early, followers)) of the paired run."""
    angles = np.ascontiguousarray(angles, dtype=np.float64)
    full, _, _, _ = _screen(engine, ref, tgt, split, angles, group, True, cull=False)
    off, t_off, y_off, items = _screen(engine, ref, tgt, split, angles, group, False)
    on, t_on, y_on, items_on = _screen(engine, ref, tgt, split, angles, group, True)
    assert np.array_equal(items, items_on)
    assert (items[:, 2] == (group if len(angles) > 1 else 1)).all(), items
    for name, w in (("switch off", off), ("switch on", on)):
        bad = np.nonzero(full.view(np.uint32) != w.view(np.uint32))[0]
        assert bad.size == 0, (name, bad[:8], full[bad[:8]], w[bad[:8]])
    assert np.array_equal(on.view(np.uint32), off.view(np.uint32))
    print("G = %d, %d rotations: tiles %d (off %d), early / followers %s (off %s)" % (group, len(angles), t_on, t_off, y_on, y_off))
    assert t_on == t_off and t_on > 0, (t_on, t_off)
    assert y_on == y_off, (y_on, y_off)
    return on, t_on, y_on


@pytest.mark.parametrize("n_angles", [1, 2, 3, 4, 8, 9, 15, 16, 17])
def test_list_lengths_at_groups_of_eight(engine, n_angles):
    """Forced G = 8, rotations 0.5 degrees apart.  1: a leader only; 2: one single follower; 3: one pair; 4: a pair and a
    single; 8: three pairs and a single; 9, 15, 16, 17: the same and a second group of each kind (16 and 17 on a second wave
    and a third)."""
    _, _, (_, fol) = _same(engine, REF3, TGT17, SPLIT3, np.radians(-4.0 + 0.5 * np.arange(n_angles)), 8)
    assert fol == n_angles - (n_angles + 7) // 8


@pytest.mark.parametrize("group, n_angles", [(2, 9), (4, 9), (4, 3)])
def test_smaller_groups(engine, group, n_angles):
    """G = 2 never pairs (one follower a group); G = 4: one pair and a single follower a group, a lone leader behind them;
    a group of three at G = 4 is a leader and one pair."""
    _, _, (_, fol) = _same(engine, REF3, TGT17, SPLIT3, np.radians(-4.0 + 0.5 * np.arange(n_angles)), group)
    assert fol == n_angles - (n_angles + group - 1) // group


def test_far_rotations(engine):
    """18 rotations 20 degrees apart at G = 8: the followers stay (tests/test_gpu_screen_cull_early.py), so every pair runs the
    general path twice, X's and then Y's."""
    _, _, (early, fol) = _same(engine, REF3, TGT17, SPLIT3, np.radians(-170.0 + 20.0 * np.arange(18)), 8)
    assert fol == 15 and early < fol


def test_flagship_pair_in_the_split_layout(engine):
    """Frame pair 1 of synthetic_pullback(12, 501): 521 + 521 points, lumen and catheter runs tile by tile (17 x 17 tiles),
    three runs of eight rotations 0.5 degrees apart."""
    _, pairs = _flagship_pairs()
    (ref, rm), (tgt, tm) = pairs[0]
    assert len(ref) == len(tgt) == 521
    angles = np.radians(np.concatenate([s + 0.5 * np.arange(8) for s in (-180.0, -60.5, 33.0)]))
    _, _, (early, fol) = _same(engine, ref, tgt, (rm, tm), angles, 8)
    assert fol == 21 and 0 < early


# (leader, X, Y) in degrees: a group of three is a leader and one pair.  Chosen on the CPU with tools/model_cull_tiles.py (a
# follower with an empty phase 2 leaves): neighbours 0.5 degrees from the leader leave, rotations 20 degrees away stay.  The
# thresholds are the group's (one circle per column tile that holds every rotation of the group), so a follower's fate is
# a property of its group: the triples are the ones whose followers have, in the model, the same fate in the triple and in
# the two-rotation list (leader, follower) that the device is asked about.
TRIPLES = [(33.0, 33.5, 34.0), (33.0, 33.5, 53.0), (33.0, 53.0, 33.5), (33.0, 53.0, 58.0),
           (0.0, 0.5, 1.0), (0.0, 20.0, 0.5), (0.0, 20.0, 25.0)]


@functools.lru_cache(maxsize=None)
def _model():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import model_cull_tiles as model
    return model


def _model_fates(deg):
    """The followers' fates of one group holding the rotations `deg` (the first leads), by the host model."""
    model = _model()
    _, p2 = model.count_tiles(REF3, TGT17, np.radians(np.asarray(deg, dtype=np.float64)), model.split_main(len(REF3), SPLIT3[0]),
                              model.split_main(len(TGT17), SPLIT3[1]), len(deg))
    return tuple("stay" if p2[k].sum() else "leave" for k in range(1, len(deg)))


def test_every_fate_of_a_pair(engine):
    """(leave, leave), (leave, stay), (stay, leave) and (stay, stay): each follower's fate is learnt from the UNPAIRED path
    (switch off, the two-rotation list leader + follower, mm_engine_screen_early), the triple then runs switch on against
    off against the full kernel.  The switch-off run of the triple must count as many early exits as the two lists say:
    the fates are then the triple's own.  The cases must hold all four combinations, on the CPU and on the device."""
    model_seen = set()
    for t in TRIPLES:
        f3 = _model_fates(t)
        assert f3 == _model_fates(t[:2]) + _model_fates((t[0], t[2])), (t, f3)
        model_seen.add(f3)
    assert len(model_seen) == 4, model_seen

    seen = set()
    for t in TRIPLES:
        fate = []
        for k in (1, 2):
            two = np.radians(np.array([t[0], t[k]]))
            _, _, (early, fol), _ = _screen(engine, REF3, TGT17, SPLIT3, two, 8, False)
            assert fol == 1 and early in (0, 1)
            fate.append("leave" if early else "stay")
        _, _, (early, fol) = _same(engine, REF3, TGT17, SPLIT3, np.radians(np.array(t)), 8)
        print(t, fate, "early exits of the triple:", early)
        assert fol == 2 and early == fate.count("leave"), (t, fate, early)
        seen.add(tuple(fate))
    assert seen == {("leave", "leave"), ("leave", "stay"), ("stay", "leave"), ("stay", "stay")}, seen


def test_stale_second_row_store(engine, mm):
    """The second row store after a 17-row-tile case holds 17 row tiles of another pair's minima: a three-row-tile case
    behind it on the same engine gives the values and counters of a fresh engine."""
    big = _set(501, 20)
    _same(engine, big, TGT17, (501, 501), np.radians(-16.0 + 2.0 * np.arange(16)), 8)
    angles = np.radians(-4.0 + 0.5 * np.arange(9))
    v, tiles, early = _same(engine, REF3, TGT17, SPLIT3, angles, 8)
    with mm.Engine() as fresh:
        w, tiles_f, early_f = _same(fresh, REF3, TGT17, SPLIT3, angles, 8)
    assert np.array_equal(v.view(np.uint32), w.view(np.uint32))
    assert tiles == tiles_f and early == early_f, (tiles, tiles_f, early, early_f)
