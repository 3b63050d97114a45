"""The culled screen's value floor as a rule, in numpy (no GPU): exact f64 squared distances stand in for the screened values,
the thresholds are those of tools/model_cull_tiles.py (tests/cull_floor_cases.py restates the rule on top of them).  For every
case the rule's value -- the largest minimum as they stand after phase 2 -- must EQUAL the brute-force largest full minimum,
for the group sizes 1, 4 and 8 with the leader's hand-over on and off, and the floor never costs a tile.

Each directed case first asserts that it is what it claims."""
import numpy as np
import pytest

import cull_floor_cases as cf

GROUPS = [(1, True), (4, True), (4, False), (8, True), (8, False)]


def _check(case, group, carry):
    """Values exact with the floor on and off; tiles with the floor never more than without.  Returns both lists."""
    ref, tgt, mains, angles = case
    off = cf.screen(ref, tgt, angles, group, carry, False, mains)
    on = cf.screen(ref, tgt, angles, group, carry, True, mains)
    for k, (a, b) in enumerate(zip(off, on)):
        assert a.value == a.brute, (k, a.value, a.brute)
        assert b.value == b.brute == a.brute, (k, b.value, b.brute)
        assert 0.0 <= b.L <= b.brute
    t_off = sum(int(c.p1.sum() + c.p2.sum()) for c in off)
    t_on = sum(int(c.p1.sum() + c.p2.sum()) for c in on)
    assert t_on <= t_off, (t_on, t_off)
    return off, on


def _random_contour(rng, n, r):
    t = np.sort(rng.uniform(0, 2 * np.pi, n))
    rr = r * (1 + 0.15 * np.sin(2 * t + rng.uniform(0, 6)) + 0.05 * rng.normal(size=n))
    return np.stack([rr * np.cos(t) + rng.normal(0, 0.1), rr * np.sin(t) * rng.uniform(0.6, 1.0)], axis=1)


@pytest.mark.parametrize("group, carry", GROUPS)
def test_random_contours(group, carry):
    rng = np.random.default_rng(1100 + group)
    fewer = 0
    for nr, nt in ((96, 521), (160, 300), (521, 521)):
        ref, tgt = _random_contour(rng, nr, rng.uniform(1.5, 3.0)), _random_contour(rng, nt, rng.uniform(1.5, 3.0))
        start = rng.uniform(-180.0, 170.0)
        off, on = _check((ref, tgt, (0, 0), np.radians(start + 0.5 * np.arange(9))), group, carry)
        fewer += sum(int(c.p2.sum()) for c in off) - sum(int(c.p2.sum()) for c in on)
    print("G = %d, hand-over %s: %d phase-2 tiles fewer with the floor" % (group, carry, fewer))


@pytest.mark.parametrize("group, carry", GROUPS)
def test_contour_sets_save_tiles(group, carry):
    """The device tests' contour case (521 target points against 96 and against 521): strictly fewer tiles with the floor."""
    for ref, mains in ((cf.REF3, (76, 501)), (cf.SET17, (501, 501))):
        off, on = _check((ref, cf.TGT17, mains, np.radians(-4.0 + 0.5 * np.arange(17))), group, carry)
        assert sum(int(c.p2.sum()) + int(c.p1.sum()) for c in on) < sum(int(c.p2.sum()) + int(c.p1.sum()) for c in off)


@pytest.mark.parametrize("group, carry", GROUPS)
def test_a_live_row_made_exact_in_phase_2_is_the_value(group, carry):
    """(a)"""
    off, on = _check(cf.case_outlier(), group, carry)
    hits = 0
    for c in on:
        i = int(np.argmax(c.fu))
        if c.fu[i] == c.value and c.fu[i] > c.fv.max() and c.u[i] > c.L and not c.srow[i] and c.fu[i] < c.u[i]:
            hits += 1
    assert hits > 0


@pytest.mark.parametrize("group, carry", GROUPS)
def test_the_floor_comes_from_a_column(group, carry):
    """(b)"""
    off, on = _check(cf.case_column_floor(), group, carry)
    hits = [c for c in on if c.L > 0 and c.v[c.scol].max(initial=0.0) == c.L > c.u[c.srow].max(initial=0.0)]
    assert hits
    # and it matters there: some row or column is not settled and stays below the floor
    assert any(((~c.srow) & (c.u <= c.L)).any() or ((~c.scol) & (c.v <= c.L)).any() for c in hits)


@pytest.mark.parametrize("group, carry", GROUPS)
def test_nothing_settled(group, carry):
    """(c) L = 0: the rule is the plain one, tile for tile."""
    off, on = _check(cf.case_nothing_settled(), group, carry)
    hits = [(a, b) for a, b in zip(off, on) if not b.srow.any() and not b.scol.any()]
    assert hits
    for a, b in hits:
        assert b.L == 0.0
        if (a.p1 == b.p1).all():
            assert (a.p2 == b.p2).all()


@pytest.mark.parametrize("group, carry", GROUPS)
def test_everything_settled(group, carry):
    """(d) phase 1 holds every tile with a thr below a minimum: no live row or column, no phase 2."""
    off, on = _check(cf.case_all_settled(), group, carry)
    hits = [c for c in on if c.srow.all() and c.scol.all()]
    assert hits
    for c in hits:
        assert not c.p2.any()
        assert c.L == max(c.u.max(), c.v.max()) == c.value


@pytest.mark.parametrize("group, carry", GROUPS)
def test_ties(group, carry):
    """(e) u_r == L exactly: the row is not live, and the value stands.  And v_c == Tc_J exactly: the column is settled.  No
    geometry gives the second tie on demand, so it is made: the smallest threshold of a column tile outside phase 1 is
    LOWERED to the minimum of one of its settled columns (a lower threshold is a valid bound too), which ties that column
    to its Tc_J."""
    ref, tgt, mains, angles = cf.case_ties()
    off, on = _check((ref, tgt, mains, angles), group, carry)
    c = on[0]
    assert c.L > 0 and int((c.u == c.L).sum() + (c.v == c.L).sum()) >= 2
    assert ((c.u == c.L) & ~c.srow).any() and ((c.v == c.L) & ~c.scol).any()
    # the made tie: the settled column with the largest minimum (the one that gave L, or its like)
    tcs = np.repeat(c.tc, 32)
    q = np.nonzero(c.scol & np.isfinite(tcs) & (c.v < tcs) & (c.v > 0))[0]
    q = int(q[np.argmax(c.v[q])])
    J = q // 32
    I = int(np.argmin(np.where(c.p1[:, J], np.inf, c.thr[:, J])))
    lower = c.thr.copy()
    assert 0.0 < c.v[q] < lower[I, J] == c.tc[J]
    lower[I, J] = c.v[q]
    for floor in (False, True):
        t = cf.candidate(c.d2, c.thr, c.p1, floor, lower)
        assert t.tc[J] == t.v[q] and t.scol[q]
        assert t.value == t.brute
    assert t.L >= t.v[q]


@pytest.mark.parametrize("group, carry", GROUPS)
def test_far_rotations_in_one_group(group, carry):
    """(f)"""
    _check(cf.case_far_group(), group, carry)


def test_model_counts_never_rise():
    """tools/model_cull_tiles.py --floor on its own protocol (a frame pair of the flagship shape, runs of eight spread over
    the list): per candidate the phase-1 tiles of a group's leader are the same and the total never exceeds the plain rule's."""
    from multimoda_rs_amd.synth import synthetic_pullback
    sets = cf.model.search_sets(synthetic_pullback(12, 501), 501)
    (ref, rm), (tgt, tm) = sets[0], sets[1]
    angles = np.radians(np.concatenate([s + 0.5 * np.arange(8) for s in (-180.0, -60.5, 33.0)]))
    rm, tm = cf.model.split_main(len(ref), rm), cf.model.split_main(len(tgt), tm)
    for group in (1, 4, 8):
        a1, a2 = cf.model.count_tiles(ref, tgt, angles, rm, tm, group, True, False)
        b1, b2 = cf.model.count_tiles(ref, tgt, angles, rm, tm, group, True, True)
        assert (a1[::group] == b1[::group]).all()
        assert b1.sum() + b2.sum() <= a1.sum() + a2.sum()
        assert ((b1 + b2).sum(axis=1)[::group] <= (a1 + a2).sum(axis=1)[::group]).all()
        print("G = %d: %d tiles, with the floor %d" % (group, a1.sum() + a2.sum(), b1.sum() + b2.sum()))
