"""The culled screen's runs on the device (k_screen_mx_cull with a run table, mm_engine_set_screen_run): a workgroup takes
consecutive work items of one pair and stages the pair -- row fragments, scaled target points, norms, circles -- at the first
of them only; a later item loads its WorkItem and its candidates' cos / sin.  A candidate must see the same operands in the
same order whichever workgroup runs its item, so every case compares, between set_screen_run(1) (a workgroup per item,
the path before runs) and each forced size,
  * the f32 BITS of every screened value, and
  * all three counters: the tiles computed (mm_engine_screen_tiles) and both words of mm_engine_screen_early.

Shapes.  The set-bit variant exists only at 17 column tiles: the two frame pairs of synthetic_pullback(3, 501), 521 + 521
points in the split layout, with set_screen_group(8), which gives work items of 32 candidates.  721 rotations: 23 items a
pair, of 31 and of 32 candidates, the last group of an item of 31 holds 7; 100 rotations: items of 25, so groups of 8, 8, 8
and 1 -- a lone candidate, and a follower without a partner.  Run sizes 2, 3, 5, 23 (the whole pair) and 64 (more than a
pair holds).  The chain variant at 16 column tiles (480 + 20 points) and at 3 (64 + 20).  Through the whole plan: the
automatic rule and a forced size on synthetic_case(12, 501) at 721 rotations against set_screen_run(1)."""
import functools
import os
import sys

import numpy as np
import pytest

from test_gpu_screen_cull_group import _set

pytestmark = pytest.mark.gpu

RUNS = (2, 3, 5, 23, 64)


@functools.lru_cache(maxsize=None)
def _pairs3():
    """The two frame pairs of synthetic_pullback(3, 501) as ((ref, main), (tgt, main))."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import model_cull_tiles as model
    from multimoda_rs_amd.synth import synthetic_pullback
    sets = model.search_sets(synthetic_pullback(3, 501), 501)
    assert len(sets) == 3 and all(len(s[0]) == 521 for s in sets)
    return [(sets[0], sets[1]), (sets[1], sets[2])]


def _angles(n):
    return np.ascontiguousarray(np.radians(-180.0 + 0.5 * np.arange(n)))


def _screen(engine, ref, tgt, split, angles, run, group=8, pair=True, floor=True):
    """(value bits, (tiles computed, followers that left early, followers), items) of one call at run size `run`."""
    engine.set_screen_run(run)
    engine.set_screen_pair(pair)
    try:
        t0, y0 = engine.screen_tiles(), engine.screen_early()
        v, _, items = engine.screen_values_floor(ref, tgt, angles, (0.0, 0.0), group, floor, split=split)
        t1, y1 = engine.screen_tiles(), engine.screen_early()
    finally:
        engine.set_screen_run(0)
        engine.set_screen_pair(True)
    return v.view(np.uint32).copy(), (t1[0] - t0[0], y1[0] - y0[0], y1[1] - y0[1]), items


_REF = {}


def _reference(engine, key, *args, **kw):
    """The run of `key` with a workgroup per item: computed once, shared, never written to."""
    if key not in _REF:
        bits, counters, items = _screen(engine, *args, 1, **kw)
        bits.setflags(write=False)
        _REF[key] = (bits, counters, items)
    return _REF[key]


def _same(engine, key, ref, tgt, split, angles, runs=RUNS, **kw):
    bits, counters, items = _reference(engine, key, ref, tgt, split, angles, **kw)
    assert counters[0] > 0
    for run in runs:
        b, c, it = _screen(engine, ref, tgt, split, angles, run, **kw)
        assert np.array_equal(it, items)
        bad = np.nonzero(b != bits)[0]
        assert bad.size == 0, (key, run, bad[:8], bits[bad[:8]], b[bad[:8]])
        assert c == counters, (key, run, c, counters)
    return counters, items


@pytest.mark.parametrize("k", [0, 1])
def test_23_items_a_pair(engine, k):
    """721 rotations: 23 items of 31 and 32 candidates, the last group of an item of 31 holds 7."""
    (ref, rm), (tgt, tm) = _pairs3()[k]
    (tiles, early, fol), items = _same(engine, ("721", k), ref, tgt, (rm, tm), _angles(721))
    assert len(items) == 23 and set(items[:, 1].tolist()) == {31, 32} and (items[:, 2] == 8).all()
    assert fol == 721 - sum((int(n) + 7) // 8 for n in items[:, 1]) and 0 < early <= fol


@pytest.mark.parametrize("k", [0, 1])
def test_items_of_25(engine, k):
    """100 rotations: four items of 25, groups of 8, 8, 8 and 1 -- a lone candidate and a follower without a partner."""
    (ref, rm), (tgt, tm) = _pairs3()[k]
    (tiles, early, fol), items = _same(engine, ("100", k), ref, tgt, (rm, tm), _angles(100))
    assert items[:, 1].tolist() == [25] * 4 and fol == 4 * 21


def test_pair_and_floor_off(engine):
    """The same comparison with the followers alone and every minimum made exact."""
    (ref, rm), (tgt, tm) = _pairs3()[0]
    for n in (721, 100):
        _same(engine, ("plain", n), ref, tgt, (rm, tm), _angles(n), pair=False, floor=False)


@pytest.mark.parametrize("lum, nct", [(480, 16), (64, 3)])
def test_chain_variant(engine, lum, nct):
    """k_screen_mx_cull<16> and <3>: items of four candidates, one a wave; a reference of other size than the target."""
    tgt = _set(lum, 20, r=2.35, phase=0.7, at=(-0.05, 0.1))
    ref = _set(53, 20)
    assert (len(tgt) + 31) // 32 == nct
    (tiles, early, fol), items = _same(engine, ("chain", nct), ref, tgt, (0, 0), _angles(100), group=1)
    assert len(items) > 5 and fol == 0


def test_whole_plan(engine, mm):
    """WithinPlan on synthetic_case(12, 501) at 721 rotations with groups of 8 (44 frame pairs of 23 items: below the
    automatic rule's limit, which must leave the launch alone) and the between-pullback rotations: the automatic rule and a
    forced size of 5 give the logs, rotations, moved pullbacks and counters of set_screen_run(1)."""
    def run(size):
        case = mm.synthetic_case(12, 501)
        engine.set_screen_run(size)
        engine.set_screen_group(8)
        try:
            t0, y0 = engine.screen_tiles(), engine.screen_early()
            plan = mm.WithinPlan(engine, case, 0.5, 180.0, True, 501, precision=mm.MM_PRECISION_F32_MATRIX)
            logs, evals, unresolved = plan.run()
            plan.close()
            a, b, c, d = case
            rot, _ = mm.align_between(engine, [(a, b), (c, d)], 180.0, 0.5, 501, mm.MM_PRECISION_F32_MATRIX)
            t1, y1 = engine.screen_tiles(), engine.screen_early()
        finally:
            engine.set_screen_run(0)
            engine.set_screen_group(0)
        return logs, evals, unresolved, list(rot), (t1[0] - t0[0], y1[0] - y0[0], y1[1] - y0[1]), [g.lumen.copy() for g in case]

    off, auto, five = run(1), run(0), run(5)
    assert off[4][0] > 0 and off[4][2] > 0
    for other in (auto, five):
        assert other[:5] == off[:5]
        for x, y in zip(other[5], off[5]):
            assert np.array_equal(x, y)


def test_setter_refuses_negative_sizes(engine, mm):
    L = mm._native.lib()
    assert L.mm_engine_set_screen_run(engine._h, -1) != 0
    assert L.mm_engine_set_screen_run(engine._h, 0) == 0
