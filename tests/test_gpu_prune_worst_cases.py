"""The two exact-f64 paths that skip work, on the inputs where skipping goes wrong.  Both claim bit-identical results to
scanning everything; a wrong bound would change a winner or a count without an error.

* Nearest neighbour (csrc/mm_ccta.cpp, csrc/mm_nn_kernels.hip): the clouds of tests/nn_worst_cases.py -- flat and
  collinear, integer grids with neighbours exactly on the radius, large offsets, duplicates across chunk borders, far
  clusters, NaN / +-inf, the slab-order and chunk-count thresholds, and one query block that only the "largest minimum
  of the block" skip rule gets right -- through nn_min_sq, symmetric_nn_distance, clean_outlier_points and the two
  scaling searches (41 morphed copies), bit for bit against the oracle.  (Their work lists are checked on the host in
  tests/test_nn_plan_host.py.)
* Winner-only Hausdorff selection (hausdorff_sets_first_min, through the test hook mm_hausdorff_first_min_state): every
  lower bound equals its numpy restatement bit for bit and is <= the oracle's cost, best / best_cost are the oracle's
  first minimum, every pair left out has bound > ub strictly, and the cases built to prune do prune."""
import math

import numpy as np
import pytest

from nn_worst_cases import cases

pytestmark = pytest.mark.gpu
NN_CASES = cases()
CAP = 4080          # max_target_points_f64(): larger sets on both sides take the bounded selection


@pytest.fixture(scope="module")
def occ(oracle):
    from oracle import oracle_ccta
    oracle_ccta.lib()
    return oracle_ccta


@pytest.fixture(scope="module")
def ocl(oracle):
    from oracle import oracle_cl
    oracle_cl.lib()
    return oracle_cl


def _same(x, y):
    return np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True)


@pytest.mark.parametrize("case", NN_CASES, ids=lambda c: c[0])
def test_nn_minima_and_counts_match_oracle(engine, mm, occ, case):
    name, a, b, r2 = case
    for q, p in ((a, b), (b, a), (a, a)):
        assert _same(mm.ccta.nn_min_sq(q, p, engine=engine), occ.nn_min_sq(q, p)), name
    assert _same(mm.ccta.symmetric_nn_distance(a, b, engine=engine), occ.symmetric_nn_distance(a, b)), name
    radius = math.sqrt(r2)
    got = mm.clean_outlier_points(a, b, radius, 0.5, engine=engine)
    exp = occ.clean_outlier_points(a, b, radius, 0.5)
    assert _same(got[0], exp[0]) and _same(got[1], exp[1]), name


def _centerline(mm, pts):
    """A straight centerline through the finite points, along their longest extent."""
    f = pts[np.isfinite(pts).all(axis=1)]
    lo, hi = f.min(axis=0), f.max(axis=0)
    ax = int(np.argmax(hi - lo))
    c = np.tile((lo + hi) / 2 + 0.37, (16, 1))
    c[:, ax] = np.linspace(lo[ax] - 1.0, hi[ax] + 1.0, 16)
    return mm.Centerline.from_contour_points(c)


@pytest.mark.parametrize("name", ["grid", "offset10000", "duplicates", "nonfinite", "block_max", "n4097x4095"])
def test_scaling_searches_match_oracle(engine, mm, occ, ocl, name):
    from helpers import to_oracle_cl
    _, a, b, _ = next(c for c in NN_CASES if c[0] == name)
    cl = _centerline(mm, a)
    ocl_ = to_oracle_cl(ocl, cl)
    best, d = mm.find_aortic_scaling(a, b, cl, engine=engine, return_distances=True)
    obest, od = occ.aortic_diameter_optimization(a, b, ocl_)
    assert best == obest and _same(d, od), name
    n_sec = len(a) // 4
    got = mm.find_proximal_distal_scaling(a, n_sec, n_sec, cl, b[:len(b) // 2], b[len(b) // 2:], engine=engine)
    exp = occ.diameter_optimization(a, n_sec, n_sec, ocl_, b[:len(b) // 2], b[len(b) // 2:])
    assert _same(got, exp), name


# ---- winner-only Hausdorff selection ------------------------------------------------------------------------------

def _bound(a, b, stride=16):
    """The selection's lower bound restated: every stride-th row of either set against all of the other, squared distances
    dx*dx + dy*dy, row minima ignoring NaN, finite minima only, the max of both directions, then sqrt."""
    def directed(x, y):
        r = x[::stride]
        with np.errstate(invalid="ignore"):
            dx = r[:, None, 0] - y[None, :, 0]
            dy = r[:, None, 1] - y[None, :, 1]
            d = dx * dx + dy * dy
        m = np.fmin.reduce(d, axis=1, initial=np.inf)
        m = m[np.isfinite(m)]
        return m.max(initial=0.0)
    return math.sqrt(max(directed(a, b), directed(b, a)))


def _pair(rng, na, nb, dist, row, off=0.0):
    """Two uniform clouds on [0, 10]^2 and one outlier of the first at `dist` beyond the edge, at index `row`: the pair's
    cost is the outlier's distance to the second cloud, which the bound sees exactly when row % 16 == 0."""
    a = rng.uniform(0.0, 10.0, (na, 2))
    b = rng.uniform(0.0, 10.0, (nb, 2))
    a[row] = (10.0 + dist, 5.0)
    return a + off, b + off


def _pair2(rng, off):
    """The worst point off the stride rows, a second outlier on one: bound (4.5) < exact (5)."""
    a, b = _pair(rng, 4352, 5120, 5.0, 5, off)
    a[32] = (14.5 + off, 5.0 + off)
    return a, b


def _move(a, src, dst):
    a = a.copy()
    a[[src, dst]] = a[[dst, src]]
    return a


def _check(engine, oracle, pairs, expect_pruned):
    st = engine.hausdorff_first_min_state(pairs)
    costs = np.array([oracle.hausdorff(a, b) for a, b in pairs])
    k = int(np.argmin(costs))                                   # the oracle's first minimum
    assert st["best"] == k and st["best_cost"] == costs[k]
    assert st["pruned"] == expect_pruned
    P = len(pairs)
    if not expect_pruned:
        assert np.isnan(st["bound"]).all() and st["pick"] == -1 and math.isnan(st["ub"])
        assert st["exact"].all() and st["n_exact"] == P
        return st, costs
    bound = np.array([_bound(a, b) for a, b in pairs])
    assert np.array_equal(st["bound"], bound)                   # bit for bit
    assert (st["bound"] <= costs).all()
    pick = int(np.argmin(bound))
    assert st["pick"] == pick and st["ub"] == costs[pick]
    assert np.array_equal(st["exact"], (bound <= costs[pick]))  # exact exactly where bound <= ub; skipped: bound > ub
    assert st["n_exact"] == int(st["exact"].sum())
    return st, costs


@pytest.mark.parametrize("off", [0.0, 1.0e5])
def test_winner_only_selection_prunes_and_keeps_ties(engine, oracle, off):
    rng = np.random.default_rng(31 if off else 30)
    # X: the pair every tie is built from; its outlier on a stride row (bound == exact) or off it (bound < exact)
    xa, xb = _pair(rng, 4353, 5121, 2.0, 0, off)
    xa[8] = (10.6 + off, 2.0 + off)                               # a milder outlier off the stride rows
    off_row, other = _move(xa, 0, 1), _move(xa, 0, 8)           # the worst point off the stride rows; other: the mild
    assert _bound(off_row, xb) < 0.6 < _bound(other, xb) < 2.0  # one on row 0 instead
    pairs = [_pair(rng, 4097, 5119, 6.0, 16, off),              # bound == exact > ub: skipped
             (xa, xb),                                          # exact == ub, bound == ub, below the pick: the tie
             _pair2(rng, off),                                  # bound < exact, both > ub: skipped
             (other, xb),                                       # permuted copy below the pick, a larger bound
             (off_row, xb),                                     # the pick: smallest bound, exact == ub
             _pair(rng, 8192, 6143, 4.0, 4096, off),
             (_move(xa, 0, 4352), xb),                          # permuted copy above the pick (the padded last row)
             _pair(rng, 8193, 6145, 7.0, 8192, off),
             (xb, xa),                                          # the same cost the other way round
             _pair(rng, 4608, 1023 + 4096, 3.0, 255 * 16, off)]
    bound = [_bound(a, b) for a, b in pairs]
    assert int(np.argmin(bound)) == 4                           # the construction does what it says
    st, costs = _check(engine, oracle, pairs, True)
    assert st["n_exact"] < len(pairs)
    assert st["best"] == 1 and costs[1] == costs[4] == st["ub"]


def test_winner_only_selection_nonfinite_rows(engine, oracle):
    rng = np.random.default_rng(32)
    pairs = []
    for k in range(9):
        a, b = _pair(rng, 4100 + 17 * k, 4200 + 255 * k, 1.0 + 0.5 * k, 16 * k + (k % 2), 0.0)
        for r, v in ((0, np.nan), (16, np.inf), (33, -np.inf), (48 + k, np.nan)):
            a[r + 100, k % 2] = v
            b[r + 200, (k + 1) % 2] = v
        pairs.append((a, b))
    st, _ = _check(engine, oracle, pairs, True)
    assert np.isfinite(st["bound"]).all()


def test_winner_only_selection_fallbacks(engine, oracle):
    rng = np.random.default_rng(33)
    big = [_pair(rng, 4081 + 40 * k, 4090 + 7 * k, 1.0 + k, 3 * k, 0.0) for k in range(8)]
    _check(engine, oracle, big[:7], False)                      # fewer than 8 pairs: every pair evaluated
    st, _ = _check(engine, oracle, big, True)                   # 8 pairs, every set above the cap
    a4080, _ = _pair(rng, CAP, 10, 0.0, 0)
    _check(engine, oracle, big[:7] + [(a4080, big[7][1])], False)   # one set of exactly 4080 points
    _check(engine, oracle, big[:7] + [(np.zeros((0, 2)), big[7][1])], False)   # one empty set
