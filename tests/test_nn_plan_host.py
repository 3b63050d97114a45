"""The work lists of the pruned nearest-neighbour launches (csrc/mm_ccta.cpp, NnPlan), checked on the host through the
test hook mm_nn_plan (no engine, no GPU) against a numpy restatement.

k_nn3_min skips a pass-B item when its lb2 is at least the largest current minimum of its queries, and k_nn3_count
launches only the items whose lb2 is within the radius.  Both are exact only if every lb2 is a true lower bound of the
squared distances the kernels compute, bit for bit, and if the lists cover every (query block, chunk) exactly once.  The
restatement uses the kernels' operation order (dx*dx + dy*dy + dz*dz, no contraction), so its distances are the
kernels' bits; the morphed sets' points are xyz + unit * adj, as k_nn3_morph computes them."""
import numpy as np
import pytest

from nn_worst_cases import SORT_MIN, cases, radial

DBL_MAX = np.finfo(np.float64).max


def _points(s):
    if isinstance(s, dict):
        return np.where(s["has"][:, None] != 0, s["xyz"] + s["unit"] * s["adj"], s["xyz"])
    return np.asarray(s, dtype=np.float64)


def _boxes(pts, qpb):
    """lo / hi of every group of qpb staged points; NaN coordinates are ignored (std::min / std::max with the running
    value first), an all-NaN group keeps (DBL_MAX, -DBL_MAX)."""
    n = len(pts)
    lo, hi = [], []
    for g0 in range(0, n, qpb):
        g = pts[g0:g0 + qpb]
        lo.append(np.fmin.reduce(g, axis=0, initial=DBL_MAX))
        hi.append(np.fmax.reduce(g, axis=0, initial=-DBL_MAX))
    return np.array(lo).reshape(-1, 3), np.array(hi).reshape(-1, 3)


def _box_lb2(alo, ahi, blo, bhi):
    """box_lb2 in its operation order: gap = max(0, max(a.lo - b.hi, b.lo - a.hi)) with std::max's NaN behaviour,
    s = ((0 + gx^2) + gy^2) + gz^2, shaved by (1 - 1e-12)."""
    s = np.float64(0.0)
    for ax in range(3):
        x, y = alo[ax] - bhi[ax], blo[ax] - ahi[ax]
        m = y if x < y else x
        gap = m if 0.0 < m else 0.0
        s = s + gap * gap
    return s * (1.0 - 1e-12)


@np.errstate(invalid="ignore")
def _d2(q, p):
    dx = q[:, None, 0] - p[None, :, 0]
    dy = q[:, None, 1] - p[None, :, 1]
    dz = q[:, None, 2] - p[None, :, 2]
    return dx * dx + dy * dy + dz * dz


def _check_plan(mm, sets, pairs, r2, order_like=None):
    plan = mm.ccta.nn_plan(sets, pairs, r2, order_like)
    qpb, ch, span = plan["qpb"], plan["chunk"], plan["span"]
    assert ch % qpb == 0 and ch // qpb == 1   # one box per chunk (gpc): the restatement below assumes it
    pts = [_points(s) for s in sets]
    for s, p in enumerate(pts):
        perm = plan["perm"][s]
        assert np.array_equal(np.sort(perm), np.arange(len(p)))        # a permutation
        if len(p) < SORT_MIN and order_like is None:
            assert np.array_equal(perm, np.arange(len(p)))              # small sets: staged as given
    staged = [p[plan["perm"][s]] for s, p in enumerate(pts)]
    boxes = [_boxes(p, qpb) for p in staged]
    la, lb, lc = plan["a"], plan["b"], plan["count"]
    n_pruned = 0
    for k, (qs, ps) in enumerate(pairs):
        Q, Pt = staged[qs], staged[ps]
        nq, np_ = len(Q), len(Pt)
        ia, ib, ic = la[la[:, 0] == k], lb[lb[:, 0] == k], lc[lc[:, 0] == k]
        lb_b, lb_c = plan["b_lb2"][lb[:, 0] == k], plan["count_lb2"][lc[:, 0] == k]
        if nq == 0 or np_ == 0:
            assert len(ia) == len(ib) == len(ic) == 0
            continue
        nqb, nch = -(-nq // qpb), -(-np_ // ch)
        # coverage: pass A and pass B together cover every (query block, chunk) exactly once
        cover = np.zeros((nqb, nch), dtype=np.int64)
        for it in np.concatenate([ia, ib]):
            assert it[1] % qpb == 0 and it[2] % ch == 0 and 0 <= it[1] < nq and 0 <= it[2] < np_
            c0 = it[2] // ch
            cover[it[1] // qpb, c0:min(nch, c0 + it[3])] += 1
        assert (cover == 1).all(), (k, np.argwhere(cover != 1)[:5])
        pruned = nq >= SORT_MIN and np_ >= SORT_MIN and nch > 2   # both staged in slab order, more than 2 chunks
        qlo, qhi = boxes[qs]
        plo, phi = boxes[ps]
        lb2 = np.array([[min(DBL_MAX, _box_lb2(qlo[b], qhi[b], plo[c], phi[c])) for c in range(nch)] for b in range(nqb)])
        # every bound, pass A's chunk included, is a lower bound of every distance of its item, bit for bit
        for b in range(nqb):
            d = _d2(Q[b * qpb:(b + 1) * qpb], Pt)
            for c in range(nch):
                blk = d[:, c * ch:(c + 1) * ch]
                m = np.fmin.reduce(blk, axis=None, initial=np.inf)          # NaN never lowers a minimum
                assert lb2[b, c] <= m, (k, b, c, lb2[b, c], m)
                if (blk <= r2).any():                                    # a neighbour within the radius is counted
                    assert ((ic[:, 1] == b * qpb) & (ic[:, 2] == c * ch)).sum() == 1, (k, b, c)
        if pruned:
            n_pruned += 1
            assert len(ia) == nqb and (ia[:, 3] == 1).all() and (ib[:, 3] == 1).all()
            assert sorted(ia[:, 1] // qpb) == list(range(nqb))              # one pass-A item per query block
            for it in ia:                                                   # ... the chunk with the smallest lb2
                b, c = it[1] // qpb, it[2] // ch
                assert lb2[b, c] == lb2[b].min() and c == int(np.argmin(lb2[b]))
            assert np.array_equal(lb_b, lb2[ib[:, 1] // qpb, ib[:, 2] // ch])    # the bits pass B compares
        else:
            assert len(ib) == 0 and (ia[:, 3] == span).all()
        # radius counts: exactly the (block, chunk) items whose lb2 is within r2, with those bounds
        want = {(b * qpb, c * ch) for b in range(nqb) for c in range(nch) if lb2[b, c] <= r2}
        assert {(int(it[1]), int(it[2])) for it in ic} == want and len(ic) == len(want)
        assert np.array_equal(lb_c, lb2[ic[:, 1] // qpb, ic[:, 2] // ch])
    return n_pruned


@pytest.mark.parametrize("case", cases(), ids=lambda c: c[0])
def test_work_lists_cover_once_and_bound_below(mm, case):
    name, a, b, r2 = case
    n_pruned = _check_plan(mm, [a, b], [(0, 1), (1, 0), (0, 0)], r2)
    if len(a) >= SORT_MIN and len(b) >= SORT_MIN:
        assert n_pruned == 3, name        # both sorted and more than 2 chunks: every pair pruned


def test_work_lists_of_morphed_sets(mm):
    """The scaling searches' layout: one reference set, morphed copies of one cloud that share the first copy's staging
    order, pairs both ways.  The host boxes the copies from Set3::at, the device moves their points itself."""
    rng = np.random.default_rng(7)
    for _, a, b, r2 in [c for c in cases() if c[0] in ("grid", "offset1e+06", "duplicates", "nonfinite", "block_max")]:
        unit, has = radial(rng, len(a))
        sets = [b] + [{"xyz": a, "unit": unit, "has": has, "adj": adj} for adj in (-2.0, -0.30000000000000004, 1.3, 2.0)]
        pairs = [p for i in range(1, len(sets)) for p in ((0, i), (i, 0))]
        order_like = [0] + [1] * (len(sets) - 1)
        assert _check_plan(mm, sets, pairs, r2, order_like) == len(pairs)


def test_plan_hook_rejects_bad_input(mm):
    with pytest.raises(Exception):
        mm.ccta.nn_plan([np.zeros((3, 3))], [(0, 1)])
    plan = mm.ccta.nn_plan([np.zeros((0, 3)), np.ones((5, 3))], [(0, 1), (1, 0)], 1.0)
    assert len(plan["a"]) == len(plan["b"]) == len(plan["count"]) == 0
