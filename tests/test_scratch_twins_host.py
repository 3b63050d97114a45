"""The builders of tests/scratch_twins.py without a device: a twin keeps the counts and changes the content, stays closed
and manifold where its original is (so an edge table holds at most a quarter of its slots: 1.5 nf edges in at least 6 nf
slots, and leftovers and new insertions together never fill one), and carries the label-independent checker results
through its permutation; a big input has at least twice the counts; and the comparison the GPU test makes
with them sees one bit in any array or field, and nothing in the fields it leaves out."""
import dataclasses

import numpy as np
import pytest

from mm_checkers import flip_edges as FE
from mm_checkers import smooth_mesh as SMO
from mm_checkers import stitch_mesh as SM
from scratch_twins import JITTER, VOLATILE, big, big_points, differences, twin, twin_perm, twin_points, uploads
from test_flip_host import SHAPES, CLOSED
from test_trim_host import capped_tube

SEEDS = (1, 2)


def face_set(f):
    return {tuple(np.roll(t, -int(np.argmin(t)))) for t in np.asarray(f).tolist()}


def edge_set(f):
    f = np.asarray(f)
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    return {tuple(x) for x in e.tolist() if x[0] != x[1]}


@pytest.mark.parametrize("name", sorted(SHAPES))
@pytest.mark.parametrize("seed", SEEDS)
def test_twin_keeps_counts_and_changes_content(name, seed):
    v, f = SHAPES[name]()
    v, f = np.asarray(v, dtype=np.float64), np.asarray(f, dtype=np.int64)
    tv, tf = twin(v, f, seed)
    perm = twin_perm(len(v), seed)
    assert tv.shape == v.shape and tf.shape == f.shape and tf.dtype == np.int64 and tv.dtype == np.float64
    assert sorted(perm.tolist()) == list(range(len(v))) and not np.array_equal(perm, np.arange(len(v)))
    assert not np.array_equal(tf, f)
    assert face_set(tf) == face_set(perm[f])                             # the same surface under other labels, windings kept
    if name not in ("tetrahedron", "octahedron"):                        # of the two solids a relabelling can be a symmetry
        assert face_set(tf) != face_set(f)
        assert edge_set(tf) - edge_set(f)                                # keys the original's table never held
    moved = np.abs(tv[perm] - v)
    assert 0.0 < moved.max() < 6 * JITTER and (moved > 0).all()
    again = twin(v, f, seed)
    assert np.array_equal(again[0], tv) and np.array_equal(again[1], tf)  # seeded
    other = twin(v, f, seed + 7)
    assert not np.array_equal(other[1], tf)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_twin_stays_closed_and_manifold_and_the_valences_follow_the_permutation(name):
    v, f = SHAPES[name]()
    f = np.asarray(f, dtype=np.int64)
    nv = len(v)
    tv, tf = twin(v, f, 1)
    perm = twin_perm(nv, 1)
    deg, border, info = FE.valence(f, nv)
    tdeg, tborder, tinfo = FE.valence(tf, nv)
    assert np.array_equal(tdeg[perm], deg) and np.array_equal(tborder[perm], border)
    assert tinfo == info
    _, n_open, n_nonmanifold = SM.face_adjacency(f)
    _, t_open, t_nonmanifold = SM.face_adjacency(tf)
    assert (t_open, t_nonmanifold) == (n_open, n_nonmanifold)
    if name in CLOSED:
        assert t_open == 0 and t_nonmanifold == 0 and tinfo["n_inconsistent_edges"] == 0
        assert 4 * tinfo["n_edges"] <= max(256, 6 * len(f))              # a quarter of the smallest table
    # the sorted adjacency rows carry over too
    off, nb, _ = SMO.csr(f, nv)
    toff, tnb, _ = SMO.csr(tf, nv)
    for k in (0, nv // 2, nv - 1):
        row = perm[nb[off[k]:off[k + 1]]]
        assert sorted(row.tolist()) == tnb[toff[perm[k]]:toff[perm[k] + 1]].tolist()


@pytest.mark.parametrize("n", [1, 255, 256, 257, 3000])
def test_twin_points(n):
    p = np.random.default_rng(n).uniform(-5, 5, (n, 3))
    t = twin_points(p, 3)
    perm = twin_perm(n, 3)
    assert t.shape == p.shape and not np.array_equal(t, p)
    assert 0.0 < np.abs(t[perm] - p).max() < 6 * JITTER
    assert np.array_equal(twin_points(p, 3), t)
    kept = twin_points(p, 3, permute=False)
    assert np.array_equal(kept, t[perm]) and np.abs(kept - p).max() < 6 * JITTER         # the same jitter, the order kept
    b = big_points(p)
    assert len(b) == 3 * n and np.array_equal(b[:n], p)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_big_has_twice_the_counts_and_stays_closed(name):
    v, f = SHAPES[name]()
    f = np.asarray(f, dtype=np.int64)
    bv, bf = big(v, f)
    assert len(bv) >= 2 * len(v) and len(bf) >= 2 * len(f) and bf.max() < len(bv) and bf.min() >= 0
    assert np.array_equal(bv[:len(v)], np.asarray(v, dtype=np.float64))
    if name in CLOSED:
        _, n_open, n_nonmanifold = SM.face_adjacency(bf)
        assert n_open == 0 and n_nonmanifold == 0
        assert FE.valence(bf, len(bv))[2]["n_inconsistent_edges"] == 0


def test_big_of_the_existing_builders():
    from test_flip_host import tube, refined_tube
    assert len(refined_tube()[0]) >= 2 * len(tube()[0]) and len(refined_tube()[1]) >= 2 * len(tube()[1])
    v, f = capped_tube(15, 17)
    assert len(v) == 257 and len(big(v, f)[1]) == 4 * len(f)


# ---- the comparison of whole results ----------------------------------------------------------------------------------------

@dataclasses.dataclass
class Report:
    distance: np.ndarray
    face: np.ndarray
    report: dict


def report():
    return {"n_flips": 7, "volume": 1.5, "bytes_uploaded": 4096, "flips_per_pass": [3, 4, 0], "items_skipped": 11,
            "winding_rounds": 5, "watertight": True}


def result():
    return ((np.arange(12.0).reshape(4, 3), np.arange(6, dtype=np.int64)),
            Report(np.array([0.5, np.nan]), np.array([1, -1]), report()), report(), [np.zeros(0)], None)


def test_the_comparison_sees_one_bit_anywhere_and_only_there():
    a = result()
    assert differences(a, result()) == [] and uploads(a) == [4096, 4096]
    b = result()
    b[0][0][2, 1] = np.nextafter(b[0][0][2, 1], 9.0)                     # one bit of one coordinate
    assert differences(a, b) == ["r[0][0]"]
    b = result()
    b[0][0][0, 0] = -0.0                                                 # equal as a number, another bit pattern
    assert differences(a, b) == ["r[0][0]"]
    b = result()
    b[1].distance[1] = -np.nan                                           # a NaN of other bits
    assert differences(a, b) == ["r[1].distance"]
    b = result()
    b[2]["volume"] = np.nextafter(1.5, 2.0)
    b[2]["flips_per_pass"][1] = 5
    b[1].report["n_flips"] = 8
    assert differences(a, b) == ["r[1].report['n_flips']", "r[2]['flips_per_pass'][1]", "r[2]['volume']"]
    b = result()
    for k in VOLATILE:                                                   # scheduling, not the input: left out
        b[2][k] = 99
    assert differences(a, b) == []
    # type, shape and structure count too
    b = result()
    assert differences(a, (b[0], b[1], b[2], [np.zeros(0, dtype=np.int64)], None)) == ["r[3][0]"]
    assert differences(a, ((b[0][0].reshape(3, 4), b[0][1]),) + b[1:]) == ["r[0][0]"]
    assert differences(a, b[:4] + (0,)) == ["r[4]"]
    assert differences(a, b[:4])[0].startswith("structure") and differences(a, b[:2] + ({"n_flips": 7},) + b[3:])[0].startswith("structure")
    assert differences((1, True, np.int32(1)), (np.int64(1), 1, 1)) == []               # an integer is its value
    assert differences((1.0,), (1,)) == ["r[0]"]
