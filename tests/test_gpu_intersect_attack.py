"""The intersection kernel (csrc/mm_intersect_kernels.hip, which compiles csrc/mm_isect_device.h for the device) on the
worst cases of tests/isect_attack_cases.py.  The cases go in as meshes of at most 512 faces, six vertices and two faces a
case, shared corners as equal coordinates; faces of different cases meet freely, which adds near-degenerate pairs of its
own (the base faces repeat, so many pairs are coincident).  Every batch: the device equals the checker's unculled scan bit
for bit (flags, pairs, states, counts, narrow_tests, the report integers); every pair it lists as intersecting meets by
the exact oracle and every intended pair it does not list is disjoint by it -- the oracle is asked about the device's
output, not the checker's.  The families without shared vertices run in the two-mesh form as well, both ways round.
A pair's state does not depend on the mesh around it: alone, in a shuffled batch, in a batch cut to 257 and 511 faces,
inside one chunk or across two.  At 2^-310 and 2^345 nothing but the box step proves anything.  Boxes that touch in one
value along x, y or z, also as -0.0 against +0.0, lose no pair.  No comparison has a tolerance."""
import numpy as np
import pytest

import isect_attack_cases as ac
from mm_checkers import mesh_intersections as X
from test_gpu_intersect import COUNTS, same_as_checker
from test_intersect_host import T

import multimoda_rs_amd as mm
from multimoda_rs_amd import intersect

pytestmark = pytest.mark.gpu

D, I, U = ac.D, ac.I, ac.U
SELF_BATCHES = [(name, b) for name in ac.FAMILIES for b in range(len(ac.batches(name)))]
NO_SHARED = {"edge_edge": ac.family("edge_edge"), "sliver": ac.family("sliver"),
             "corner": tuple(c for c in ac.family("corner") if ac.n_shared(c) == 0)}
TWO_BATCHES = [(name, b) for name in NO_SHARED for b in range(-(-len(NO_SHARED[name]) // ac.BATCH_CASES))]


def _faces(v, f, with_ids):
    tri = [T(*t) for t in v[f]]
    ids = X.canonical_ids(v)[f] if with_ids else f
    return tri, [tuple(int(x) for x in r) for r in ids]


def _listed(got):
    return {tuple(p): int(s) for p, s in zip(got.pairs.tolist(), got.pair_state.tolist())}


def run_self(engine, v, f, intended):
    """The self form against the checker and the oracle; intended: the pairs (i, j) that a case put there.  Returns the
    result and the state of every intended pair."""
    got = same_as_checker(mm.mesh_self_intersections((v, f), engine=engine), X.scan(v, f), len(f), 0, True)
    tri, ids = _faces(v, f, True)
    listed = _listed(got)
    for (i, j), s in listed.items():
        assert i < j and s in (I, U)
        if s == I:
            assert ac.meets(tri[i], tri[j], ids[i], ids[j]), (tri[i], tri[j])
    for i, j in intended:
        if (i, j) not in listed:
            assert not ac.meets(tri[i], tri[j], ids[i], ids[j]), (tri[i], tri[j])
    return got, [listed.get(p, D) for p in intended]


def run_two(engine, va, fa, vb, fb, intended):
    got = same_as_checker(mm.mesh_intersections((va, fa), (vb, fb), engine=engine), X.scan_two(va, fa, vb, fb), len(fa), len(fb),
                          False)
    (ta, _), (tb, _) = _faces(va, fa, False), _faces(vb, fb, False)
    listed = _listed(got)
    for (i, j), s in listed.items():
        if s == I:
            assert ac.meets(ta[i], tb[j], (0, 1, 2), (3, 4, 5)), (ta[i], tb[j])
    for i, j in intended:
        if (i, j) not in listed:
            assert not ac.meets(ta[i], tb[j], (0, 1, 2), (3, 4, 5)), (ta[i], tb[j])
    return got, [listed.get(p, D) for p in intended]


def _intended(n):
    return [(2 * k, 2 * k + 1) for k in range(n)]


@pytest.mark.parametrize("name, b", SELF_BATCHES, ids=["%s-%d" % nb for nb in SELF_BATCHES])
def test_self_form_batches(engine, name, b):
    cases = ac.batches(name)[b]
    v, f = ac.pack(cases)
    assert len(f) <= 512
    got, state = run_self(engine, v, f, _intended(len(cases)))
    assert state == [ac.rule_state(*c[:4]) for c in cases]                # equal coordinates recreate the ids of the case
    print(name, b, "intended pairs disjoint / intersecting / undecided:", ac.counts(state), "of all pairs:",
          {k: got.report[k] for k in COUNTS})


@pytest.mark.parametrize("name, b", TWO_BATCHES, ids=["%s-%d" % nb for nb in TWO_BATCHES])
def test_two_mesh_batches_both_ways_round(engine, name, b):
    cases = NO_SHARED[name][b * ac.BATCH_CASES:(b + 1) * ac.BATCH_CASES]
    pairs = [(k, k) for k in range(len(cases))]
    _, state = run_two(engine, *ac.pack_two(cases), pairs)
    assert state == [ac.rule_state(c[0], c[1]) for c in cases]
    _, swapped = run_two(engine, *ac.pack_two(cases, swapped=True), pairs)
    assert swapped == [ac.rule_state(c[1], c[0]) for c in cases]
    print(name, b, "a against b:", ac.counts(state), "b against a:", ac.counts(swapped))


def mixed_batch():
    """256 cases drawn evenly from the constructed families, in an order that mixes them."""
    every = [c for name in ac.BUILT for c in ac.family(name)]
    cases = [every[k * len(every) // ac.BATCH_CASES] for k in range(ac.BATCH_CASES)]
    order = np.random.default_rng(5).permutation(len(cases))
    return [cases[k] for k in order]


def test_a_pairs_state_does_not_depend_on_its_batch(engine):
    cases = mixed_batch()
    n = len(cases)
    assert n == ac.BATCH_CASES
    v, f = ac.pack(cases)
    got, state = run_self(engine, v, f, _intended(n))
    assert state == [ac.rule_state(*c[:4]) for c in cases] and min(ac.counts(state)) >= 20
    # the arrangement: both chunks against themselves and against each other, intended pairs of either kind
    assert got.report["items"] == got.report["items_total"] == 3
    where = np.argsort(intersect.isect_plan((v, f))["order_a"]) // X.CHUNK
    inside = [k for k in range(n) if where[2 * k] == where[2 * k + 1]]
    across = [k for k in range(n) if where[2 * k] != where[2 * k + 1]]
    assert min(len(inside), len(across)) >= 20
    for group in (inside, across):
        assert sum(state[k] != D for k in group) >= 10
    # alone
    alone = [k for k in range(n) if state[k] != D][:96]
    assert len(alone) >= 64 and {state[k] for k in alone} == {I, U}
    for k in alone:
        one = mm.mesh_self_intersections(ac.pack(cases[k:k + 1]), engine=engine)
        assert one.pairs.tolist() == [[0, 1]] and one.pair_state.tolist() == [state[k]], cases[k]
        assert one.report["narrow_tests"] == 1
    # shuffled: a pair keeps its state under its new indices, with the face of the lower index as face 1 where the
    # order survives; where it is reversed the state is that of the reversed pair
    perm = np.random.default_rng(9).permutation(len(f))
    inv = np.argsort(perm)
    mixed = mm.mesh_self_intersections((v, f[perm]), engine=engine)
    listed = _listed(mixed)
    reversed_pairs = 0
    for k in range(n):
        i, j = int(inv[2 * k]), int(inv[2 * k + 1])
        c = cases[k]
        if i < j:
            assert listed.get((i, j), D) == state[k]
        else:
            reversed_pairs += 1
            assert listed.get((j, i), D) == ac.rule_state(c[1], c[0], c[3], c[2])
    assert 0 < reversed_pairs < n
    for key in ("narrow_tests", "n_coincident_pairs", "n_degenerate_faces", "items"):
        assert mixed.report[key] == got.report[key], key
    # cut to one face past a chunk and to one face short of two
    for nf in (257, 511):
        part, part_state = run_self(engine, v, f[:nf], _intended(nf // 2))
        assert part_state == state[:nf // 2] and part.report["items_total"] == 3


@pytest.mark.parametrize("k", ac.SCALE_ENDS)
def test_the_ends_of_the_scale_prove_nothing_but_by_boxes(engine, k):
    cases = ac.scaled(k)
    undecided = 0
    for c in cases:                                                       # a case alone: its two faces and nothing else
        v, f = ac.pack([c])
        one = same_as_checker(mm.mesh_self_intersections((v, f), engine=engine), X.scan(v, f), 2, 0, True)
        assert one.report["n_intersecting_pairs"] == 0 and one.report["n_undecided_pairs"] == one.report["narrow_tests"]
        assert one.pair_state.tolist() == [U] * one.report["narrow_tests"]
        if one.report["narrow_tests"] == 0:                               # disjoint by the box step alone: truly disjoint
            assert not ac.meets(*c[:4])
        undecided += one.report["n_undecided_pairs"]
    assert undecided > len(cases) // 2
    # the cases as one batch: faces repeat, and a face against itself is coincident at any scale; nothing else intersects
    v, f = ac.pack(cases)
    got, state = run_self(engine, v, f, _intended(len(cases)))
    assert got.report["n_intersecting_pairs"] == got.report["n_coincident_pairs"] and I not in state
    tri, _ = _faces(v, f, True)
    for (i, j), s in _listed(got).items():
        assert s == U or sorted(tri[i]) == sorted(tri[j])
    print("2^%d: %d cases alone, %d undecided, the others apart by their boxes; as a batch" % (k, len(cases), undecided),
          {key: got.report[key] for key in COUNTS})


@pytest.fixture(scope="module")
def touching_at_one(engine):
    v, f = ac.touching_mesh()
    return mm.mesh_self_intersections((v, f), engine=engine)


@pytest.mark.parametrize("at, signed_zeros, ax", ac.TOUCHING_MESHES, ids=ac.TOUCHING_IDS)
def test_boxes_that_touch_in_one_value_lose_no_pair(engine, touching_at_one, at, signed_zeros, ax):
    v, f = ac.touching_mesh(at, signed_zeros, ax)
    n = ac.TOUCHING
    got = same_as_checker(mm.mesh_self_intersections((v, f), engine=engine), X.scan(v, f), 2 * n, 0, True)
    assert got.pairs.tolist() == [[k, n + k] for k in range(n)] and (got.pair_state == U).all()
    assert got.report["narrow_tests"] == n and got.report["n_undecided_pairs"] == n and got.report["items"] == 3
    assert (got.face_state == U).all()
    for arr in ("face_state", "pairs", "pair_state"):
        assert np.array_equal(getattr(got, arr), getattr(touching_at_one, arr))
    assert got.report == touching_at_one.report
    two = same_as_checker(mm.mesh_intersections((v, f[:n]), (v, f[n:]), engine=engine), X.scan_two(v, f[:n], v, f[n:]), n, n,
                          False)
    assert two.pairs.tolist() == [[k, k] for k in range(n)] and (two.pair_state == U).all()
    assert two.report["narrow_tests"] == n and two.report["items"] == two.report["items_total"] == 1
    back = same_as_checker(mm.mesh_intersections((v, f[n:]), (v, f[:n]), engine=engine), X.scan_two(v, f[n:], v, f[:n]), n, n,
                           False)
    assert back.pairs.tolist() == [[k, k] for k in range(n)] and back.report["narrow_tests"] == n


def test_a_face_degenerate_by_rounding(engine):
    v, f = ac.rounding_degenerate_mesh()
    got = same_as_checker(mm.mesh_self_intersections((v, f), engine=engine), X.scan(v, f), 3, 0, True)
    assert got.report["n_degenerate_faces"] == 1 and got.report["narrow_tests"] == 1
    assert got.pairs.tolist() == [[0, 1]] and got.pair_state.tolist() == [I] and got.face_state.tolist() == [1, 1, 0]
    two = same_as_checker(mm.mesh_intersections((v, f[:1]), (v, f[1:]), engine=engine), X.scan_two(v, f[:1], v, f[1:]), 1, 2,
                          False)
    assert two.report["n_degenerate_faces"] == 1 and two.report["narrow_tests"] == 1 and two.pairs.tolist() == [[0, 0]]
