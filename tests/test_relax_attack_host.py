"""The mesh relaxation on the worst cases of tests/relax_attack_cases.py, without a device: the rule as
tests/mm_checkers/relax_mesh.py states it (the unpruned scan) against tests/relax_exact.py, an oracle in rational arithmetic
that shares no operation with it.  tests/test_gpu_relax_attack.py runs the same assertions (check_result, skip_claim) on
what the device returns.

(b) On the surface.  Every free vertex with ref_face >= 0 lies, by its exact distance, within on_surface_bound of the
    face it reports; no vertex is exempt.  ref_face == -1 for no free vertex, but for all of them at 2^600.
(c) Nearest and lowest, where the query is the input vertex (iterations == 0): ref_face is one of the faces whose exact
    distance is within the allowance of the exact minimum, and the lowest of them where they are all copies of one
    triangle.  The allowance is that of tests/test_surface_sliver_host.py (test_fold_against_the_exact_nearest): the
    largest altitude of a thin face plus R_TOL * max(D, M).  In the tie family ref_face is nearest_exact's face, and after
    any number of iterations no vertex reports a face that has a copy of lower index.
(d) The exact grid: z is +0.0 bit for bit; a vertex the oracle keeps is within the bound of (b) of the exact candidate
    (the step is exact: only the projection rounds), one it takes back has its input bits; n_reverted and
    n_flipped_faces are the oracle's counts.  Every sign the oracle decides is at least 2^-12 of dot(m_old, m_old) from
    zero, forty binary orders above the projection's rounding.
(e) The skip claim.  An item (query block, chunk) of an iteration must be skipped where the exact gap between the
    block's box of candidates and the chunk's box is strictly above the block's largest exact distance from a candidate
    to the result it starts from -- the face it had before the step.  That distance is the minimum the device holds for
    the query when the item decides (the seed), so the device skips such an item whatever the order its items run in; a
    distance to the face a candidate ends on is reached only after other items have run, and no order is promised.  The
    gaps of these cases exceed the distances by units, the slack (64 ulp of the largest coordinate) by far less.  Every
    refreshed bound, as relax_mesh.refreshed_items restates it, is at most every d2 of its item as the rule computes
    them, and at most the exact d2 of the item's nearest pair.

Worst on-surface ratios measured on the CPU (distance / bound; test_rule_on_the_attack_cases prints each): the largest is
0.334 (offset_2p20_project), then 0.28 (offset_2p36_project) and 0.25 (seed_cap_random); the ties 0.09, the stale and
wide cases below 0.11.
"""
import functools
import math
from fractions import Fraction

import numpy as np
import pytest

import relax_attack_cases as AC
import relax_exact as EX
from mm_checkers import relax_mesh as RX
from mm_checkers import surface_distance as S
from test_refine_host import same_bits
from test_surface_sliver_host import R_TOL, exact_altitude, scale_of

from multimoda_rs_amd import surface

SKIP_FAMILIES = ("stale", "wide", "offset", "scale")
GRID_MARGIN = 2.0 ** -12


def arrays(case):
    """(v, f, rv, rf, pinned, iterations, lambda) with the mesh as its own reference where the case names none."""
    _, (v, f), ref, pinned, iterations, lamb = case
    v, f = np.asarray(v, dtype=np.float64), np.asarray(f, dtype=np.int64)
    rv, rf = (v, f) if ref is None else (np.asarray(ref[0], dtype=np.float64), np.asarray(ref[1], dtype=np.int64))
    return v, f, rv, rf, pinned, iterations, lamb


@functools.lru_cache(maxsize=None)
def checked(name):
    """The checker's answer for a case, computed once for both files: (vertices, ref_face, report, trace)."""
    v, f, rv, rf, pinned, iterations, lamb = arrays(AC.cases()[name])
    return RX.relax(v, f, rv, rf, iterations=iterations, lamb=lamb, pinned=pinned, trace=True)


@functools.lru_cache(maxsize=None)
def free_of(name):
    v, f, _, _, pinned, _, _ = arrays(AC.cases()[name])
    return RX.classify(f, len(v), pinned)[0]


def on_surface_bound(tri, x):
    """R_TOL * max(D, M) of the face and the point (tests/test_surface_sliver_host.py): the closest point the rule
    returns is a corner's bits, u + e t, or (a + ab v) + ac w with v, w, v + w within rounding of [0, 1].  An error in t,
    v or w moves the point inside the face's plane or along its edge; what leaves the face is the rounding of the
    differences, products and sums that build the point, each at most half an ulp of a value no larger than M."""
    return R_TOL * scale_of(tri, x)


@functools.lru_cache(maxsize=None)
def lowest_copy(name):
    """Per reference face, the lowest index of a face with the same three corner indices in the same order."""
    rf = arrays(AC.cases()[name])[3]
    first = {}
    return np.array([first.setdefault(tuple(t), k) for k, t in enumerate(rf.tolist())], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def thin_allowance(name):
    rv, rf = arrays(AC.cases()[name])[2:4]
    alts = [exact_altitude(*rv[t]) for t in rf if S.face_kind(rv, t) == S.THIN]
    return max(alts) if alts else 0.0


@functools.lru_cache(maxsize=None)
def grid_oracle(name):
    v, f, _, _, _, _, lamb = arrays(AC.cases()[name])
    return EX.grid_step_exact(v, f, free_of(name), lamb)


_verified = {}


def check_result(name, x, face, rep):
    """(b), (c), (d) and the tie rule on one result of the case -- the checker's or the device's.  Returns the worst
    on-surface ratio.  A result with the bits of one already verified is not verified again."""
    key = (np.ascontiguousarray(x).tobytes(), np.ascontiguousarray(face).tobytes(), rep["n_reverted"], rep["n_flipped_faces"])
    if _verified.get(name, (None,))[0] == key:
        return _verified[name][1]
    v, f, rv, rf, pinned, iterations, lamb = arrays(AC.cases()[name])
    free = free_of(name)
    idx = np.flatnonzero(free)
    assert rep["n_free"] == len(idx) > 0
    assert same_bits(x[~free], v[~free]) and (face[~free] == -1).all()
    # (b)
    lost = int((face[idx] < 0).sum())
    if name == "scale_2p600":
        assert lost == len(idx) and same_bits(x, v)
    else:
        assert lost == 0, (name, lost)
    worst = 0.0
    for i in idx[face[idx] >= 0]:
        tri = rv[rf[face[i]]]
        bound = on_surface_bound(tri, x[i])
        d2 = EX.dist2_exact(x[i], *tri)
        assert d2 <= Fraction(bound) ** 2, (name, int(i), int(face[i]), math.sqrt(d2), bound)
        worst = max(worst, math.sqrt(d2) / bound)
    # the tie rule, after any number of iterations
    if AC.family(name) == "ties":
        low = lowest_copy(name)
        assert (low[face[idx]] == face[idx]).all(), (name, "a face with a copy of lower index")
    # (c)
    if iterations == 0:
        used = rv[np.unique(rf)]
        allow = thin_allowance(name) + R_TOL * scale_of(used, v[idx])
        tol = R_TOL * scale_of(used, v[idx])
        low = lowest_copy(name)
        decided = 0
        for i in idx:
            best, lowest, exact = EX.nearest_exact(v[i], rv, rf, tol)
            near = sorted(k for k, d in exact.items() if math.sqrt(d) <= math.sqrt(best) + allow)
            assert int(face[i]) in near, (name, int(i), int(face[i]), near)
            if len({int(low[k]) for k in near}) == 1:
                decided += 1
                assert int(face[i]) == near[0] == lowest, (name, int(i), int(face[i]), near)
            if AC.family(name) == "ties":
                assert int(face[i]) == lowest, (name, int(i), int(face[i]), lowest)
        print(f"{name}: face decided by the exact distances for {decided} of {len(idx)} vertices")
        assert decided > len(idx) // 4
    # (d)
    if AC.family(name) == "grid":
        cand, reverted, flipped, margin = grid_oracle(name)
        assert margin >= GRID_MARGIN
        assert (x[:, 2].view(np.uint64) == 0).all()
        for i in idx:
            i = int(i)
            if i in reverted:
                assert same_bits(x[i], v[i]), (name, i)
            else:
                bound = on_surface_bound(rv[rf[face[i]]], x[i])
                off = sum((Fraction(float(x[i, a])) - cand[i][a]) ** 2 for a in range(3))
                assert off <= Fraction(bound) ** 2, (name, i, math.sqrt(off), bound)
        assert rep["n_reverted"] == len(reverted) and rep["n_flipped_faces"] == flipped, (name, len(reverted), flipped)
    _verified[name] = (key, worst)
    return worst


@functools.lru_cache(maxsize=None)
def skip_claim(name):
    """(e): (the plan of step 0, per iteration the number of items that must be skipped, per iteration the items as
    (q0, c0, exact gap squared, the block's largest exact seed distance squared or None))."""
    v, f, rv, rf, _, _, _ = arrays(AC.cases()[name])
    free = free_of(name)
    steps = checked(name)[3]
    plan = surface.tri_plan(v[free], (rv, rf))
    perm, qpb, ch = plan["query_perm"], plan["qpb"], plan["chunk"]
    corners = rv[rf[plan["face_order"]]]
    counts, listed = [], []
    for st in steps:
        cand, prev = st["candidates"][perm], st["faces_before"][perm]
        items = []
        for q0 in range(0, len(cand), qpb):
            blk, was = cand[q0:q0 + qpb], prev[q0:q0 + qpb]
            top = None
            if (was >= 0).all():
                top = max(EX.dist2_exact(p, *rv[rf[k]]) for p, k in zip(blk, was))
            qlo, qhi = EX.fr(blk.min(axis=0)), EX.fr(blk.max(axis=0))
            for c0 in range(0, len(corners), ch):
                pts = corners[c0:c0 + ch].reshape(-1, 3)
                clo, chi = EX.fr(pts.min(axis=0)), EX.fr(pts.max(axis=0))
                gap2 = sum(max(0, qlo[a] - chi[a], clo[a] - qhi[a]) ** 2 for a in range(3))
                items.append((q0, c0, gap2, top))
        counts.append(sum(1 for _, _, gap2, top in items if top is not None and gap2 > top))
        listed.append(items)
    return plan, counts, listed


# ---- the cases hold what they say ----------------------------------------------------------------------------------------

def test_the_cases_hold_what_they_say():
    cases = AC.cases()
    assert len(cases) == len(AC.NAMES) == 33
    # ties: the index order survives, so a face and its copy lie in different chunks; some teeth have no copy
    for name in ("ties_0", "ties_shuffled_0"):
        v, f, rv, rf, _, _, _ = arrays(cases[name])
        low = lowest_copy(name)
        assert len(rf) == 2 * AC.TEETH + AC.LONE and int((low != np.arange(len(rf))).sum()) == AC.TEETH
        plan = surface.tri_plan(v[free_of(name)], (rv, rf))
        assert np.array_equal(plan["face_order"], np.arange(len(rf))) and plan["chunk"] == AC.CHUNK
        copies = np.flatnonzero(low != np.arange(len(rf)))
        across = int((copies // AC.CHUNK != low[copies] // AC.CHUNK).sum())
        assert across == AC.TEETH if name == "ties_0" else across > AC.TEETH // 2
        if name == "ties_0":
            assert (copies - low[copies] >= AC.CHUNK).all()
    v, f, rv, rf, _, _, _ = arrays(cases["ties_filled_0"])                # the sorted plan: borders part 44 and 38 pairs
    low = lowest_copy("ties_filled_0")
    assert len(rf) == 2 * (2 * AC.FILLED - 1) and (np.flatnonzero(low != np.arange(len(rf))) - 299 == low[299:]).all()
    where = np.argsort(surface.tri_plan(v[free_of("ties_filled_0")], (rv, rf))["face_order"]) // AC.CHUNK
    parted = np.flatnonzero(where[:299] != where[299:])
    assert len(parted) > 60 and {0, 1, 2} == set(where[parted].tolist()) | set(where[parted + 299].tolist())
    near = rf[parted][:, 0]                                               # the apex index = the tooth: under the grids
    assert ((near >= 100) & (near < 146)).sum() > 10
    # stale and wide: 513 and 512 free vertices, three chunks
    for name, n_free in (("stale_up", 513), ("stale_down_twice", 513), ("wide_8", 512), ("wide_64", 512)):
        rf = arrays(cases[name])[3]
        assert int(free_of(name).sum()) == n_free and 2 * AC.CHUNK < len(rf) <= 3 * AC.CHUNK
    for name in AC.NAMES:
        if AC.family(name) in ("offset", "scale"):
            assert int(free_of(name).sum()) == 257 and len(arrays(cases[name])[3]) == 510
    # seeds: the kinds of the previous faces
    for fam in ("needle_axis", "cap_random", "collinear"):
        _, _, rv, rf, _, _, _ = arrays(cases[f"seed_{fam}"])
        kinds = {S.face_kind(rv, t) for t in rf}
        assert S.THIN in kinds and (S.PROPER in kinds or fam == "collinear")
        assert int(free_of(f"seed_{fam}").sum()) == 528
    rv, rf = arrays(cases["seed_degenerate"])[2:4]
    assert [S.face_kind(rv, t) for t in rf[:3]] == [S.DEGENERATE] * 3


def test_seeds_are_what_the_cases_say():
    """The previous faces of the seed cases: degenerate ones, thin ones on either side of the rule, and the one whose d2
    for the candidate is NaN."""
    x, face, rep, steps = checked("seed_degenerate")
    before = steps[0]["faces_before"]
    assert set(before.tolist()) == {0, 1, 2}
    for fam in ("needle_axis", "cap_random", "collinear"):
        rv, rf = arrays(AC.cases()[f"seed_{fam}"])[2:4]
        kinds = np.array([S.face_kind(rv, t) for t in rf])
        before = checked(f"seed_{fam}")[3][0]["faces_before"]
        assert (before >= 0).all() and S.THIN in set(kinds[before].tolist())
    v, f, rv, rf, pinned, _, _ = arrays(AC.cases()["seed_nan"])
    x, face, rep, steps = checked("seed_nan")
    free = free_of("seed_nan")
    assert (steps[0]["faces_before"] == 0).all() and not steps[0]["stays"].any()
    t = rf[0]
    with np.errstate(all="ignore"):
        q = S.closest_on_face(steps[0]["candidates"], rv[t[0]], rv[t[1]], rv[t[2]], S.face_kind(rv, t))[0]
        assert np.isnan(S.dist_sq(steps[0]["candidates"], q)).all()       # the seed is not a number: it stays at +inf
    assert (face[free] > 0).all() and rep["n_free"] == 6                  # the floor took them


# ---- (b) (c) (d) on the checker's output -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", AC.NAMES)
def test_rule_on_the_attack_cases(name):
    x, face, rep, steps = checked(name)
    worst = check_result(name, x, face, rep)
    moved = sum(int((~st["stays"]).sum()) for st in steps)
    print(f"{name}: {rep['n_free']} free, worst on-surface ratio {worst:.3f} of the bound, {moved} candidates moved, "
          f"reverted {rep['n_reverted']}, flipped {rep['n_flipped_faces']}")
    assert worst <= 1.0


def test_the_cases_are_not_vacuous():
    # ties: candidates change face, some from a tooth without a copy to one with a copy, and every copy loses
    for name in ("ties_1", "ties_shuffled_3"):
        rf = arrays(AC.cases()[name])[3]
        low = lowest_copy(name)
        has_copy = np.isin(np.arange(len(rf)), low[low != np.arange(len(rf))])
        free = free_of(name)
        start, end = checked(name[:-1] + "0")[1][free], checked(name)[1][free]
        changed = start != end
        from_lone = changed & ~has_copy[start] & has_copy[end]
        print(f"{name}: {int(changed.sum())} of {len(start)} vertices changed face, {int(from_lone.sum())} from a tooth "
              f"without a copy to one with a copy, {int(has_copy[end].sum())} end on a face that has a copy")
        assert changed.sum() > 10 and from_lone.sum() > 0 and has_copy[end].sum() > 50
    free = free_of("ties_filled_3")
    assert (checked("ties_filled_0")[1][free] != checked("ties_filled_3")[1][free]).sum() > 10
    # stale: the winners of step 0 and of the iteration lie in different chunks
    for name in ("stale_up", "stale_down_twice"):
        plan = skip_claim(name)[0]
        where = np.argsort(plan["face_order"]) // plan["chunk"]
        free = free_of(name)
        x, face, rep, steps = checked(name)
        assert rep["n_reverted"] == 0
        assert set(where[steps[0]["faces_before"]].tolist()) == {1}
        assert set(where[face[free]].tolist()) == ({2} if name == "stale_up" else {0})
    # wide: R is thrown, and alone
    for name in ("wide_8", "wide_64"):
        v = arrays(AC.cases()[name])[0]
        free = free_of(name)
        st = checked(name)[3][0]
        r = int(np.flatnonzero(np.flatnonzero(free) == AC.ROGUE[name])[0])
        far = np.abs(st["candidates"][:, 2] - v[free][:, 2])
        assert far[r] > (2.5 if name == "wide_8" else 25.0) and np.delete(far, r).max() < 0.05
    # the grid: some lambda reverts, some does not
    reverts = {name: len(grid_oracle(name)[1]) for name in AC.NAMES if AC.family(name) == "grid"}
    flips = {name: grid_oracle(name)[2] for name in reverts}
    print("grid: reverted", reverts, "flipped", flips)
    assert min(reverts.values()) == 0 and max(reverts.values()) > 0


# ---- (e) the skip claim and the refreshed bounds -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", [n for n in AC.NAMES if AC.family(n) in SKIP_FAMILIES and AC.cases()[n][4] > 0])
def test_refreshed_bounds_and_must_skip_counts(name):
    v, f, rv, rf, _, iterations, _ = arrays(AC.cases()[name])
    free = free_of(name)
    steps = checked(name)[3]
    plan, counts, listed = skip_claim(name)
    qpb, ch = plan["qpb"], plan["chunk"]
    sf = rf[plan["face_order"]]
    n_items = -(-int(free.sum()) // qpb) * -(-len(rf) // ch)
    assert len(counts) == iterations
    for st, exact_items in zip(steps, listed):
        cand = st["candidates"][plan["query_perm"]]
        pairs = S.pair_sq(cand, rv, sf)                                   # (staged face, staged query), as the rule computes
        items = RX.refreshed_items(plan, st, rv, rf)
        assert len(items) == len(exact_items) == n_items
        for (q0, c0, lb2, top), (eq0, ec0, gap2, etop) in zip(items, exact_items):
            assert (q0, c0) == (eq0, ec0)
            block = pairs[c0:c0 + ch, q0:q0 + qpb]
            if np.isnan(block).all():
                continue
            assert lb2 <= np.nanmin(block), (name, q0, c0)
            if np.isfinite(np.nanmin(block)):
                k, q = np.unravel_index(np.nanargmin(block), block.shape)
                assert Fraction(lb2) <= EX.dist2_exact(cand[q0 + q], *rv[sf[c0 + k]]), (name, q0, c0)
                assert Fraction(lb2) <= gap2
            if etop is not None and gap2 > etop:                          # what must be skipped, the restated rule skips
                assert lb2 >= top, (name, q0, c0)
    print(f"{name}: {n_items} items an iteration, must skip {counts}")
    if AC.family(name) == "stale":
        assert all(n > 0 for n in counts)
    if name == "wide_64":                                                 # the block's box covers every chunk
        assert counts == [0] and all(lb2 == 0.0 for _, _, lb2, _ in RX.refreshed_items(plan, steps[0], rv, rf))
