"""The culled screen's candidate groups on the device (k_screen_mx_cull at 17 column tiles with WorkItem::pad = G): a wave
takes G consecutive candidates, builds thr and the phase-1 masks once for them from circles that hold a column tile under
every rotation of the group (mm_tile_group_circle), and the group's first candidate hands its phase-2 tiles to the others,
which run them in phase 1.  Every case asserts, for G = 2, 4 and 8:
  * the screened values are BIT-identical to the full kernel's and to the culled kernel's with G = 1;
  * `done` (the tiles computed) lies in the bracket of the group rule restated in numpy.

The bracket.  The rule is evaluated on the plan's work items (first candidate, candidates, G), which
mm_screen_values_group reports: a wave's groups are the runs [q G, (q + 1) G) of an item.  thr of a group comes from the
kernel's own f32 code on the host (mm_tile_bound_probe_group).  The phase-1 minima are f64 squared distances taken at -/+ the
screen's error bound, as in tests/test_gpu_screen_cull_dispatch.py; with the hand-over the uncertainty of the leader's
phase-2 mask carries into the followers' phase 1, so the bracket keeps two masks, C_lo <= carry <= C_hi:
  lower count of a follower: the tiles of m1 | C_lo, and every other tile whose thr is below the phase-1 maxima of the
      LARGER mask m1 | C_hi less e2 (a tile of C_hi not handed over is then computed in phase 2: counted either way);
  upper count: the tiles of m1 | C_hi, and every other tile whose thr is not above the maxima of the SMALLER mask plus e2.
Where the leader's mask is certain both collapse to the plain rule."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
GROUPS = (2, 4, 8)
P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


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
    assert L.mm_tile_slot_map(int(n), int(take), len(out), P(out)) == take
    return out, take


def _thr_group(mm, ref, tgt, mains, angles, e, e2):
    """thr[nrt, nct] of one group of rotations, by the kernel's own f32 code run on the host."""
    rx, ry = (np.ascontiguousarray(ref[:, k], dtype=np.float32) for k in (0, 1))
    tx, ty = (np.ascontiguousarray(tgt[:, k], dtype=np.float32) for k in (0, 1))
    nrt, nct = (len(rx) + 31) // 32, (len(tx) + 31) // 32
    circ = np.zeros(4 * (nrt + nct), dtype=np.float32)
    thr = np.zeros(nrt * nct, dtype=np.float32)
    cs = np.ascontiguousarray(np.stack([np.cos(angles), np.sin(angles)], axis=1), dtype=np.float32)
    rc = mm._native.lib().mm_tile_bound_probe_group(P(rx), P(ry), len(rx), P(tx), P(ty), len(tx), int(mains[0]), int(mains[1]),
                                                    int(e), P(cs), len(cs), float(e2), P(circ), P(thr))
    assert rc == 0
    return thr.reshape(nrt, nct).astype(np.float64)


def _phase1(thr):
    close = ~(thr > 0)
    m1 = close.copy()
    for i in np.nonzero(~close.any(axis=1))[0]:
        m1[i, np.argmin(thr[i])] = True
    for j in np.nonzero(~close.any(axis=0))[0]:
        m1[np.argmin(thr[:, j]), j] = True
    return m1


def _group_bounds(mm, ref, tgt, split, angles, items, detail=None):
    """(lower, upper) count of the tiles the group rule computes over the work items (module docstring).  detail (a list):
    per group (m1, C_lo, C_hi) is appended."""
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

    lo = hi = 0
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
                sure = ~p_lo & (thr < maxima(d2, p_hi) - e2s)
                maybe = ~p_hi & ~(thr > maxima(d2, p_lo) + e2s)
                lo += int(p_lo.sum()) + int(sure.sum())
                hi += int(p_hi.sum()) + int(maybe.sum())
                if k == 0:
                    c_lo, c_hi = sure, maybe
                    if detail is not None:
                        detail.append((m1, c_lo, c_hi))
    return lo, hi


def _run(engine, ref, tgt, angles, split, group, cull=True):
    t0 = engine.screen_tiles()
    if group is None:
        v, e2 = engine.screen_values(ref, tgt, angles, (0.0, 0.0), cull=cull, split=split)
        items = None
    else:
        v, e2, items = engine.screen_values_group(ref, tgt, angles, (0.0, 0.0), group, cull=cull, split=split)
    t1 = engine.screen_tiles()
    return v, e2, t1[0] - t0[0], t1[1] - t0[1], items


def _same(engine, mm, ref, tgt, split, angles, groups=GROUPS, detail=None):
    """Full kernel, G = 1 and every G of `groups`: values, totals, brackets.  Returns {G: tiles done} (1: per candidate)."""
    angles = np.ascontiguousarray(angles, dtype=np.float64)
    full, e2a, _, _, _ = _run(engine, ref, tgt, angles, split, None, cull=False)
    one, e2b, done1, total, _ = _run(engine, ref, tgt, angles, split, None)
    assert e2a == e2b and total == len(angles) * ((len(ref) + 31) // 32) * ((len(tgt) + 31) // 32)
    bad = np.nonzero(full.view(np.uint32) != one.view(np.uint32))[0]
    assert bad.size == 0, (bad[:8], full[bad[:8]], one[bad[:8]])
    done = {1: done1}
    for G in groups:
        v, e2g, dn, tot, items = _run(engine, ref, tgt, angles, split, G)
        assert e2g == e2a and tot == total
        bad = np.nonzero(full.view(np.uint32) != v.view(np.uint32))[0]
        assert bad.size == 0, (G, bad[:8], full[bad[:8]], v[bad[:8]])
        # the items cover the list in order, with the group size asked for
        assert (items[:, 2] == (G if len(angles) > 1 else 1)).all()
        assert items[0, 0] == 0 and (items[1:, 0] == items[:-1, 0] + items[:-1, 1]).all() and items[:, 1].sum() == len(angles)
        lo, hi = _group_bounds(mm, ref, tgt, split, angles, items.tolist(), detail if G == groups[-1] else None)
        print("G = %d: tiles done %d of %d (per candidate: %d), the group rule's count in [%d, %d], items %s" %
              (G, dn, tot, done1, lo, hi, items[:, 1].tolist()))
        assert 0 < dn <= tot and lo <= dn <= hi, (G, dn, lo, hi)
        done[G] = dn
    return done


def _lumen(n, r=2.3, phase=0.0, squash=0.8):
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    rr = r * (1 + 0.08 * np.sin(3 * t + phase) + 0.04 * np.cos(5 * t - phase))
    return np.stack([rr * np.cos(t), squash * rr * np.sin(t)], axis=1)


def _catheter(n, at=(0.1, -0.05)):
    u = np.linspace(0, 2 * np.pi, n, endpoint=False) + 0.3
    return np.stack([at[0] + 0.5 * np.cos(u), at[1] + 0.5 * np.sin(u)], axis=1)


def _set(lum, cath, r=2.3, phase=0.0, at=(0.1, -0.05)):
    return np.concatenate([_lumen(lum, r, phase), _catheter(cath, at)])


REF3, TGT17 = _set(53, 20), _set(501, 20, r=2.35, phase=0.7, at=(-0.05, 0.1))


@pytest.mark.parametrize("n_angles", [1, 7, 8, 9, 33])
def test_mixed_tile_counts(engine, mm, n_angles):
    """501 + 20 target against 53 + 20 reference (17 x 3 tiles), candidates 0.5 degrees apart.  One candidate; 7: a partial
    group at G = 8, a lone leader behind full groups at G = 2; 8; 9: a lone leader behind a full group of eight, a lone
    follower (a group of two) nowhere but at G = 2; 33: several work items (a forced G asks for items of 4 G candidates),
    groups on every wave and partial groups at their ends."""
    _same(engine, mm, REF3, TGT17, (53, 501), np.radians(-4.0 + 0.5 * np.arange(n_angles)))


@pytest.mark.parametrize("kind", ["20 degrees apart", "shuffled"])
def test_forced_groups_of_far_rotations(engine, mm, kind):
    """Nothing in the bound needs close or ordered angles: forced groups of rotations 20 degrees apart and of a shuffled
    list give the same values; they only cost tiles (the bracket is the same rule)."""
    ang = -170.0 + 20.0 * np.arange(18)
    if kind == "shuffled":
        ang = np.random.default_rng(6).permutation(np.linspace(-180.0, 180.0, 19))
    done = _same(engine, mm, REF3, TGT17, (53, 501), np.radians(ang))
    assert done[8] >= done[1]


def _ellipse(n, a=8.0, b=1.0):
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    return np.stack([a * np.cos(t), b * np.sin(t)], axis=1)


def _clusters17():
    """tests/test_gpu_screen_cull_dispatch.py: 17 column tiles, each a cluster of 32 points: 15 along the reference ellipse,
    one far above arc 1 and one far left of arc 2 -- two lone column tiles."""
    rng = np.random.default_rng(17)
    t = np.linspace(0, 2 * np.pi, 15, endpoint=False) + 0.2
    mid = np.concatenate([1.01 * np.stack([8.0 * np.cos(t), np.sin(t)], axis=1), [(-2.0, 12.0), (-16.0, 0.0)]])
    return (mid[:, None, :] + rng.normal(0, 0.02, (17, 32, 2))).reshape(544, 2)


CLUSTER_ANGLES = np.radians(-2.0 + 0.5 * np.arange(9))


@pytest.mark.parametrize("n_ref", [160, 544])
def test_lone_tiles_and_the_hand_over(engine, mm, n_ref):
    """The 17-column clusters against the ellipse at 5 and 17 row tiles, nine candidates 0.5 degrees apart (a group of eight
    and a lone leader at G = 8).  Checked on the CPU first: the group's table has lone column tiles and, at 17 row tiles, a
    row tile with no close tile; and the leader of the group of eight has phase-2 tiles for certain (C_lo), which its
    followers then take in phase 1."""
    ref, tgt = _ellipse(n_ref), _clusters17()
    e, e2 = _scale(ref, tgt)
    thr = _thr_group(mm, ref, tgt, (0, 0), CLUSTER_ANGLES[:8], e, e2)
    assert (thr > 0).all(axis=0).any() and (~(thr > 0)).any()
    if n_ref == 544:
        assert (thr > 0).all(axis=1).any()
    detail = []
    lo, hi = _group_bounds(mm, ref, tgt, (0, 0), CLUSTER_ANGLES, [(0, 9, 8)], detail)
    m1, c_lo, c_hi = detail[0]
    assert c_lo.any() and not (c_lo & m1).any() and lo <= hi
    _same(engine, mm, ref, tgt, (0, 0), CLUSTER_ANGLES)


def _flagship_pairs():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import model_cull_tiles as model
    from multimoda_rs_amd.synth import synthetic_pullback
    sets = model.search_sets(synthetic_pullback(12, 501), 501)
    return model, [(sets[i - 1], sets[i]) for i in (1, 2, 3, 4)]


def test_cost_cap_on_the_flagship_shape(engine, mm):
    """Frame pairs 1 - 4 of synthetic_pullback(12, 501), three runs of eight rotations 0.5 degrees apart: the tiles at G = 8
    stay below 1.15 x the tiles at G = 1, on the device and in the model (tools/model_cull_tiles.py gives 1.07 as the mean
    over 15 runs; the margin is for the spread from pair to pair)."""
    model, pairs = _flagship_pairs()
    angles = np.radians(np.concatenate([s + 0.5 * np.arange(8) for s in (-180.0, -60.5, 33.0)]))
    dev = {1: 0, 8: 0}
    mod = {1: 0, 8: 0}
    for (ref, rm), (tgt, tm) in pairs:
        done = _same(engine, mm, ref, tgt, (rm, tm), angles, groups=(8,))
        for G in (1, 8):
            dev[G] += done[G]
            p1, p2 = model.count_tiles(ref, tgt, angles, model.split_main(len(ref), rm), model.split_main(len(tgt), tm), G)
            mod[G] += int(p1.sum() + p2.sum())
    print("tiles G = 8 / G = 1: device %.3f (%d / %d), model %.3f" % (dev[8] / dev[1], dev[8], dev[1], mod[8] / mod[1]))
    assert mod[8] < 1.15 * mod[1], mod
    assert dev[8] < 1.15 * dev[1], dev


def test_within_plan_switch(engine, mm):
    """WithinPlan on the benchmark's `tiny` workload (4 pullbacks x 12 frames x 501 + 20 points, 181 rotations 2 degrees
    apart): logs and moved pullbacks are identical with the switch automatic, off and forced to 2, and a resident plan keeps
    the setting it was staged with (forced 2 at staging, off afterwards: the tile count of forced 2)."""
    def run(create, later):
        case = mm.synthetic_case(12, 501)
        engine.set_screen_group(create)
        try:
            plan = mm.WithinPlan(engine, case, 2.0, 180.0, True, 501, precision=mm.MM_PRECISION_F32_MATRIX)
            engine.set_screen_group(later)
            t0 = engine.screen_tiles()
            logs, evals, unresolved = plan.run()
            t1 = engine.screen_tiles()
            plan.close()
        finally:
            engine.set_screen_group(0)
        return logs, evals, unresolved, t1[0] - t0[0], t1[1] - t0[1], [g.lumen.copy() for g in case]

    auto, off, two, kept = run(0, 0), run(1, 1), run(2, 2), run(2, 1)
    assert auto[:3] == off[:3] == two[:3] == kept[:3]
    for a, b, c, d in zip(auto[5], off[5], two[5], kept[5]):
        assert np.array_equal(a, b) and np.array_equal(a, c) and np.array_equal(a, d)
    assert auto[4] == off[4] == two[4] == kept[4] > 0
    print("tiny: tiles done automatic %d, off %d, forced 2 %d, staged with 2 and run with off %d, of %d" %
          (auto[3], off[3], two[3], kept[3], off[4]))
    assert 0 < off[3] <= off[4] and 0 < two[3] <= two[4]
    assert kept[3] == two[3] != off[3]


def test_setter_refuses_other_values(engine, mm):
    L = mm._native.lib()
    for bad in (-1, 3, 5, 16):
        assert L.mm_engine_set_screen_group(engine._h, bad) != 0
    assert L.mm_engine_set_screen_group(engine._h, 0) == 0
