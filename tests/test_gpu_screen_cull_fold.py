"""The culled screen's leaner tile and check steps (k_screen_mx_cull: mxc_fold's eight minima as compiled, the paired tile
step's indexed reads, a pair's row and column minima met X with Y in one swap, one store for both row stores): bookkeeping
only, so every case asserts
  * the screened values BIT-identical (the f32 bits) to the full kernel's (set_screen_cull off), with the pair switch on and
    with it off, with the value floor on and with it off;
  * the three counters -- mm_engine_screen_tiles' computed tiles and both words of mm_engine_screen_early, followers that left
    after phase 1 and all followers -- equal, exactly, pair switch on against off.

The shapes are the ones at which a body of the kernel is reached that the other culled-screen tests reach rarely or not at all:
the last column tile's own register and tail bodies at 17 x 17 tiles, phase 2 through the set-bit loop for followers that stay,
the chain variant's unrolled bodies one column tile below the set-bit variant, and last tiles that hold a single point."""
import os
import re

import numpy as np
import pytest

from test_gpu_screen_cull_group import _set

pytestmark = pytest.mark.gpu

NEAR = np.radians(-4.0 + 0.5 * np.arange(16))       # a leader, three pairs, a single follower, a short second group (G = 8)
FAR = np.radians(-170.0 + 20.0 * np.arange(16))     # followers stay: phase 2 through the set-bit loop


def _setbit_min_nct():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "multimoda-rs_amd", "csrc", "mm_screen_limits.h")) as f:
        return int(re.search(r"kMxCullSetbitMinNct\s*=\s*(\d+)", f.read()).group(1))


def _screen(engine, ref, tgt, split, angles, group, pair, floor, cull=True):
    """(values, (tiles computed, followers that left early, followers)) of one call."""
    engine.set_screen_pair(pair)
    try:
        t0, y0 = engine.screen_tiles(), engine.screen_early()
        v, _, _ = engine.screen_values_floor(ref, tgt, angles, (0.0, 0.0), group, floor, cull=cull, split=split)
        t1, y1 = engine.screen_tiles(), engine.screen_early()
    finally:
        engine.set_screen_pair(True)
    return v, (t1[0] - t0[0], y1[0] - y0[0], y1[1] - y0[1])


def _same(engine, ref, tgt, split, angles, group=8):
    """Pair switch on against off against the full kernel, the floor off and on.  Returns the counters of (floor off, on)."""
    angles = np.ascontiguousarray(angles, dtype=np.float64)
    full, _ = _screen(engine, ref, tgt, split, angles, group, True, False, cull=False)
    out = []
    for floor in (False, True):
        off, c_off = _screen(engine, ref, tgt, split, angles, group, False, floor)
        on, c_on = _screen(engine, ref, tgt, split, angles, group, True, floor)
        for name, w in (("pair off", off), ("pair on", on)):
            bad = np.nonzero(full.view(np.uint32) != w.view(np.uint32))[0]
            assert bad.size == 0, (name, "floor", floor, bad[:8], full[bad[:8]], w[bad[:8]])
        print("floor %d: tiles, early, followers %s (pair off %s)" % (floor, c_on, c_off))
        assert c_on == c_off and c_on[0] > 0, (floor, c_on, c_off)
        out.append(c_on)
    return out


@pytest.fixture(scope="module")
def pairs521():
    """Frame pairs 1 and 2 of synthetic_pullback(3, 501): 521 + 521 points, lumen and catheter runs tile by tile."""
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import model_cull_tiles as model
    from multimoda_rs_amd.synth import synthetic_pullback
    sets = model.search_sets(synthetic_pullback(3, 501), 501)
    assert all(len(p) == 521 for p, _ in sets)
    return [(sets[0], sets[1]), (sets[1], sets[2])]


@pytest.mark.parametrize("which", [0, 1])
@pytest.mark.parametrize("kind", ["near", "far"])
def test_seventeen_by_seventeen(engine, pairs521, which, kind):
    """Case A.  17 x 17 tiles, forced G = 8.  near: 16 rotations 0.5 degrees apart -- a leader, three pairs, a single follower
    and a short second group on another wave; the last column tile's own register and the tail bodies are reached.  far: 16
    rotations 20 degrees apart -- the followers stay and phase 2 runs through the set-bit loop."""
    (ref, rm), (tgt, tm) = pairs521[which]
    (t0, early0, fol0), (t1, early1, fol1) = _same(engine, ref, tgt, (rm, tm), NEAR if kind == "near" else FAR)
    assert fol0 == fol1 == 14
    if kind == "near":
        assert 0 < early0 and 0 < early1
    else:
        assert early0 < fol0                        # (somebody stays: phase 2 of a follower)
    assert t1 <= t0                                 # (the floor only takes tiles away)


@pytest.mark.parametrize("below", [0, 1])
@pytest.mark.parametrize("kind", ["near", "far"])
def test_smallest_setbit_size_and_the_chain_below_it(engine, below, kind):
    """Case B.  The smallest target the set-bit variant takes, kMxCullSetbitMinNct column tiles with one point in the last,
    and the largest the chain variant takes, one column tile less and every tile full: its unrolled bodies.  Three row tiles,
    the last partly filled; 16 rotations."""
    nct = _setbit_min_nct() - below
    n_tgt = 32 * nct if below else 32 * (nct - 1) + 1
    ref, tgt = _set(53, 20), _set(n_tgt - 20, 20, r=2.35, phase=0.7, at=(-0.05, 0.1))
    assert (len(tgt) + 31) // 32 == nct and len(ref) == 73
    (_, _, fol0), (_, _, fol1) = _same(engine, ref, tgt, (0, 0), NEAR if kind == "near" else FAR)
    assert fol0 == fol1 == (0 if below else 14)     # (the chain variant knows no groups)


@pytest.mark.parametrize("kind", ["near", "far"])
def test_last_tiles_of_one_point(engine, kind):
    """Case C.  n = 32 k + 1 on both sides, consecutive points: 65 reference points (three row tiles) and 513 target points
    (17 column tiles), the last tile of each a single point and 31 empty slots."""
    ref, tgt = _set(45, 20), _set(493, 20, r=2.35, phase=0.7, at=(-0.05, 0.1))
    assert len(ref) == 65 and len(tgt) == 513
    _same(engine, ref, tgt, (0, 0), NEAR if kind == "near" else FAR)
    _same(engine, tgt, _set(493, 20), (0, 0), (NEAR if kind == "near" else FAR)[:9])      # 17 x 17, both last tiles one point
