"""The pruning claims of MM_PRECISION_F32_BOUNDED (the default precision of every `mm.from_*` call) on worst-case inputs.

The bounded search returns the oracle's winner only if every candidate it rules out really costs more than the winner.
A bound that is slightly too high or a chord that is slightly too short crashes nothing: it drops the true winner on the
inputs where it matters, and the search returns another rotation without an error.  So the claims are checked one by
one, against the oracle's f64 costs `oc`, on the constructions of the directed error search (tests/mx_worst_cases.py)
at the sizes the bound rounds take, at three scales, in both orientations, for both bound families (matrix pipe and
packed FMA):
  * round 1 (test hook mm_lower_bounds): sqrt(max(lb - e2, 0)) - delta <= oc for every candidate, and lb IS the bound of
    its queries (numpy) up to the kernel's error -- a bound that is valid but useless fails;
  * the state every round leaves (test hook mm_bound_state): a finite final bound is a lower bound (rounds 4 and 5);
    a candidate the chord rule ruled out (bound +inf) costs more than the first pick; one that did not survive costs
    more than the better pick; every index at the minimum cost survives; every screened value is within e2 of oc^2;
  * the first pick's row and column minima (test hook mm_pick_minima) within e2 of numpy;
  * end to end, with every round run (bound_stats: `offered` = candidates): winner index, angle and cost bit-equal to
    the oracle's.
A 'rotated copy' construction makes the cost exactly as steep as the chord rule assumes, next to a candidate of the first
round: there a chord that is too short rules out the winner.  The largest fraction of e2 the kernels use is appended to
$MM_TEST_RECORD_DIR/bound_error_bound.jsonl when that variable is set."""
import json
import os

import numpy as np
import pytest

from mx_worst_cases import angles_far_from_unit_norm, cases

pytestmark = pytest.mark.gpu
U = 2.0 ** -24
SCALES = [1.0, 2.0 ** -7, 3.0e4]
MAX_REF = 528          # k_screen_lb / k_screen_mx_emit keep a reference set of up to 16 x 33 rows (max_rows_fast)


def _takes(ref, tgt, matrix):
    """Whether the bounded search runs its bound rounds on this pair (include/mm_hausdorff.h, mm_bound_state)."""
    nr, nt = len(ref), len(tgt)
    if not (64 <= nr <= MAX_REF and nt >= 64):
        return False
    return nt <= 544 if matrix else True


def _rotated_copy(rng, n, r=500.0, k=5):
    """k tight clusters of points at radius ~r (72 degrees apart), and the same set rotated by -THETA: the cost of a
    candidate D away from THETA is r * 2 sin(|D| / 2), exactly the chord k_lb_spread allows for, as far as 8 candidates."""
    j = np.arange(n)
    phi = 2 * np.pi * (j % k) / k + 0.1 + 1e-7 * (j // k)
    rad = r * (1.0 - 1e-3 * rng.uniform(0, 1, n))
    ref = np.stack([rad * np.cos(phi), rad * np.sin(phi)], 1)
    c, s = np.cos(-THETA), np.sin(-THETA)
    return ref, np.stack([ref[:, 0] * c - ref[:, 1] * s, ref[:, 0] * s + ref[:, 1] * c], 1)


# candidates 0.02 rad apart with the optimum at index 25: one step after the sparse round's candidate 24, seven before 32
STEP_ANGLES = -0.5 + 0.02 * np.arange(65)
THETA = STEP_ANGLES[25]


def _bound_cases():
    """(name, ref, tgt, angles): the directed search's constructions at the sizes the bound rounds take, both orientations
    (a 544-point set is the target against the first 528 points of the other), radii far apart either way, and the rotated
    copy; plus the pairs they must refuse (name starts with 'refuse')."""
    rng = np.random.default_rng(20240)
    angles = np.sort(np.concatenate([angles_far_from_unit_norm(), np.linspace(-np.pi, np.pi, 33)[:-1], [0.0]]))
    out = []
    for name, a, b in cases(rng):
        n = len(a)
        if n == 600:
            out.append((f"refuse {name}", a, b, angles))
            continue
        if n == 544:
            out.append((f"refuse-ref>{MAX_REF} {name}", a, b, angles))
        out.append((name, a[:MAX_REF], b, angles))
        out.append((f"{name} swapped", b[:MAX_REF], a, angles))
    rng = np.random.default_rng(4)
    for n in (64, 223, 449, 528):
        big = _rotated_copy(rng, n)[0]
        small = big * 2.0 ** -6 + rng.normal(0, 0.5, big.shape)
        out.append((f"ra<<rb n={n}", small, big, angles))
        out.append((f"ra>>rb n={n}", big, small, angles))
        ref, tgt = _rotated_copy(rng, n)
        out.append((f"rotated-copy n={n}", ref, tgt, STEP_ANGLES))
        out.append((f"rotated-copy n={n} swapped", tgt, ref, -STEP_ANGLES))
    return out


def _strided_bound(ref, tgt, angles, stride):
    """The squared bound of round 1's queries in f64: every stride-th point of either set against all of the other."""
    want = []
    for th in angles:
        cs, sn = np.cos(th), np.sin(th)
        rt = np.stack([tgt[:, 0] * cs - tgt[:, 1] * sn, tgt[:, 0] * sn + tgt[:, 1] * cs], 1)
        d1 = ((ref[::stride][:, None, :] - rt[None, :, :]) ** 2).sum(2).min(1).max()
        d2 = ((rt[::stride][:, None, :] - ref[None, :, :]) ** 2).sum(2).min(1).max()
        want.append(max(d1, d2))
    return np.array(want)


def check_state(st, oc, name):
    """The claims of rounds 2 - 7 against the exact costs; returns the largest |screened - oc^2| / e2."""
    lb, sq, (c1, c2), e2, delta = st["lb"].astype(np.float64), st["sq"].astype(np.float64), st["picks"], st["e2"], st["delta"]
    n = len(oc)
    assert 0 <= c1 < n and 0 <= c2 < n, (name, c1, c2)
    fin = np.isfinite(lb)
    assert np.all(np.isfinite(lb) | (lb == np.inf)), name
    assert np.all(np.sqrt(np.maximum(lb[fin] - e2, 0.0)) - delta <= oc[fin]), f"{name}: a final bound above the exact cost"
    assert np.all(oc[~fin] > oc[c1]), f"{name}: the chord rule ruled out {np.flatnonzero(~fin & (oc <= oc[c1]))[:8]}"
    kept = np.isfinite(sq)
    assert np.all(np.isfinite(sq) | (sq == np.inf)), name
    assert kept[c1] and kept[c2], f"{name}: a pick did not survive"
    assert np.all(oc[~kept] > min(oc[c1], oc[c2])), f"{name}: dropped {np.flatnonzero(~kept & (oc <= min(oc[c1], oc[c2])))[:8]}"
    assert np.all(kept[oc == oc.min()]), f"{name}: a candidate at the minimum cost did not survive"
    s = sq[kept]
    lo, hi = np.sqrt(np.maximum(s - e2, 0.0)) - delta, np.sqrt(s + e2) + delta
    assert np.all((oc[kept] >= lo) & (oc[kept] <= hi)), f"{name}: a screened value outside its interval"
    frac = float(np.abs(s - oc[kept] ** 2).max() / e2)
    assert frac < 1.0, (name, frac)
    return frac


@pytest.mark.parametrize("matrix", [True, False])
@pytest.mark.parametrize("scale", SCALES)
def test_bound_rounds_on_worst_cases(engine, oracle, mm, scale, matrix):
    worst = {"round1_frac_of_e2": 0.0, "round1_lb_over_oc2_frac": 0.0, "final_lb_over_oc2_frac": 0.0, "screened_frac_of_e2": 0.0}
    n_checked = n_refused = n_ruled_out = n_dropped = 0
    for name, ref, tgt, angles in _bound_cases():
        ref, tgt = ref * scale, tgt * scale
        if name.startswith("refuse"):
            assert not _takes(ref, tgt, matrix), name
            with pytest.raises(RuntimeError):
                engine.bound_state(ref, tgt, angles, (0.0, 0.0), matrix=matrix)
            with pytest.raises(RuntimeError):
                engine.lower_bounds(ref, tgt, angles, (0.0, 0.0), matrix=matrix)
            n_refused += 1
            continue
        oc = oracle.costs_over_angles(ref, tgt, angles, 0.0, 0.0)
        ra, rb = np.hypot(ref[:, 0], ref[:, 1]).max(), np.hypot(tgt[:, 0], tgt[:, 1]).max()
        rho = ra + rb
        # ---- round 1 ----
        lb, e2, delta, stride = engine.lower_bounds(ref, tgt, angles, (0.0, 0.0), matrix=matrix)
        lb = lb.astype(np.float64)
        assert np.all(np.isfinite(lb)), name
        assert np.all(np.sqrt(np.maximum(lb - e2, 0.0)) - delta <= oc), f"{name}: a round-1 bound above the exact cost"
        want = _strided_bound(ref, tgt, angles, stride)
        err = np.abs(lb - want).max()
        assert err <= e2 + 2 * delta * rho + 1e-300, f"{name}: not the bound of its queries ({err / e2:.3g} e2)"
        if err / e2 > worst["round1_frac_of_e2"]:
            worst.update(round1_frac_of_e2=float(err / e2), round1_case=name)
        worst["round1_lb_over_oc2_frac"] = max(worst["round1_lb_over_oc2_frac"], float(np.max(lb - oc ** 2) / e2))
        # ---- every round ----
        st = engine.bound_state(ref, tgt, angles, (0.0, 0.0), matrix=matrix)
        assert st["e2"] == e2 and st["delta"] == delta, name
        frac = check_state(st, oc, name)
        fin = np.isfinite(st["lb"])
        if fin.any():
            worst["final_lb_over_oc2_frac"] = max(worst["final_lb_over_oc2_frac"],
                                                  float(np.max(st["lb"][fin].astype(np.float64) - oc[fin] ** 2) / e2))
        if frac > worst["screened_frac_of_e2"]:
            worst.update(screened_frac_of_e2=frac, screened_case=name)
        n_ruled_out += int((~fin).sum())
        n_dropped += int((~np.isfinite(st["sq"])).sum())
        # ---- end to end: every round run, the oracle's winner bit for bit ----
        (bi, ba, bc), stats = _bounded(engine, matrix, lambda: engine.best_rotation(
            ref, tgt, angles, (0.0, 0.0), skip_zero=True, precision=mm.MM_PRECISION_F32_BOUNDED))
        assert stats["offered"] == len(angles), (name, stats)
        w = int(np.argmin(oc))
        assert bi == w and ba == angles[w] and bc == oc[w], (name, bi, w, bc, oc[w])
        n_checked += 1
    worst.update(scale=scale, matrix=matrix, cases=n_checked, refused=n_refused, ruled_out=n_ruled_out, dropped=n_dropped)
    record = os.environ.get("MM_TEST_RECORD_DIR")          # where to keep the measured fractions, if anywhere
    if record:
        os.makedirs(record, exist_ok=True)
        with open(os.path.join(record, "bound_error_bound.jsonl"), "a") as f:
            f.write(json.dumps(worst) + "\n")
    assert n_checked >= 100 and n_refused >= 13
    assert n_ruled_out > 0 and n_dropped > 0                # the chord rule and the last round did prune something
    # the contract: no bound kernel error reaches e2 (the lb - oc^2 fractions are recorded only: they include delta's share)
    assert worst["round1_frac_of_e2"] < 1.0 and worst["screened_frac_of_e2"] < 1.0, worst


@pytest.mark.parametrize("scale", SCALES)
def test_pick_minima_on_worst_cases(engine, scale):
    angles = [0.0, *angles_far_from_unit_norm()[[3, 60]]]
    n = 0
    for name, ref, tgt, _ in _bound_cases():
        if name.startswith("refuse") or not _takes(ref, tgt, True) or name.endswith("swapped"):
            continue
        ref, tgt = ref * scale, tgt * scale
        for th in angles:
            rows, cols, val, e2 = engine.pick_minima(ref, tgt, th, (0.0, 0.0), skip_zero=False)
            cs, sn = np.cos(th), np.sin(th)
            rt = np.stack([tgt[:, 0] * cs - tgt[:, 1] * sn, tgt[:, 0] * sn + tgt[:, 1] * cs], 1)
            d2 = ((ref[:, None, :] - rt[None, :, :]) ** 2).sum(2)
            assert np.abs(rows - d2.min(1)).max() <= e2, f"{name} angle {th}: row minima"
            assert np.abs(cols - d2.min(0)).max() <= e2, f"{name} angle {th}: column minima"
            assert val == max(rows.max(), cols.max()), name
            n += 1
    assert n > 100


def _bounded(engine, matrix, fn):
    """fn() with every bound round run (no minimum batch size) on the asked family; the switches are restored."""
    try:
        engine.set_bound_min_candidates(0)
        engine.set_bound_matrix(matrix)
        engine.profile(True)
        out = fn()
        stats = engine.bound_stats()
    finally:
        engine.profile(False)
        engine.set_bound_min_candidates(16384)
        engine.set_bound_matrix(True)
    return out, stats


def _lists(rng):
    """Candidate lists the chord rule and the sparse round rarely see."""
    base = STEP_ANGLES
    perm = rng.permutation(len(base))
    dup = np.repeat(base[::3], 2)[:40]
    uneven = np.sort(np.concatenate([THETA + rng.normal(0, 0.004, 9), rng.uniform(-np.pi, np.pi, 30)]))
    out = [("unsorted", base[perm]), ("duplicated", dup), ("duplicated-unsorted", dup[rng.permutation(len(dup))]),
           ("non-uniform", uneven), ("optimum-duplicated", np.concatenate([base[:26], [THETA, THETA], base[26:]]))]
    for k in (1, 2, 3, 5, 7, 9, 10, 17, 18, 25, 26, 65, 66):       # n_ang < 8 and n_ang = 1, 2 (mod 8)
        out.append((f"n_ang={k}", np.linspace(THETA - 0.02 * (k // 3), THETA + 0.02 * (k - 1 - k // 3), k)))
    out.append(("with-zero", np.concatenate([[0.0], base[:30], [0.0]])))
    return out


@pytest.mark.parametrize("matrix", [True, False])
@pytest.mark.parametrize("skip_zero", [True, False])
def test_candidate_lists_the_rounds_rarely_see(engine, oracle, mm, matrix, skip_zero):
    rng = np.random.default_rng(9)
    centre = (3.25, -1.5)                                  # off the origin: a rotation by 0.0 rounds unless it is skipped
    sets = []
    for n in (64, 449, 528):
        ref, tgt = _rotated_copy(rng, n, r=40.0)
        sets.append((f"rotated-copy n={n}", ref + centre, tgt + centre))
    t = cases(np.random.default_rng(20240))
    sets += [(nm, a[:MAX_REF] / 8 + centre, b / 8 + centre) for nm, a, b in t if len(a) == 449 and "ties" in nm][:2]
    for sname, ref, tgt in sets:
        for lname, angles in _lists(rng):
            name = f"{sname} {lname} skip_zero={skip_zero}"
            oc = oracle.costs_over_angles(ref, tgt, angles, *centre, between=not skip_zero)
            st = engine.bound_state(ref, tgt, angles, centre, skip_zero=skip_zero, matrix=matrix)
            check_state(st, oc, name)
            (bi, ba, bc), stats = _bounded(engine, matrix, lambda: engine.best_rotation(
                ref, tgt, angles, centre, skip_zero=skip_zero, precision=mm.MM_PRECISION_F32_BOUNDED))
            assert stats["offered"] == len(angles), (name, stats)
            w = int(np.argmin(oc))
            assert bi == w and ba == angles[w] and bc == oc[w], (name, bi, w, bc, oc[w])


@pytest.mark.parametrize("matrix", [True, False])
def test_batch_of_directed_pairs_sharing_one_column_tile_count(engine, oracle, mm, matrix):
    """Several pairs in one launch of every round, targets of 449 .. 480 points (15 column tiles), references of every
    size the rounds take, worst-case constructions mixed with rotated copies; each pair against the oracle."""
    rng = np.random.default_rng(31)
    t = [x for x in cases(np.random.default_rng(20240)) if len(x[1]) == 449]
    refs, tgts, lists, centres = [], [], [], []
    for i, (nm, a, b) in enumerate(t[:6]):
        nr = (64, 223, 449, 300, 528, 97)[i]
        refs.append(np.concatenate([a, b])[:nr] * 2.0 ** -5)
        tgts.append(np.concatenate([b, a])[: 449 + 5 * i] * 2.0 ** -5)
        lists.append(np.sort(np.concatenate([angles_far_from_unit_norm(40), rng.uniform(-0.3, 0.3, 9 + i)])))
        centres.append((0.0, 0.0))
    for n in (64, 300, 528):
        ref, tgt = _rotated_copy(rng, 460)
        refs.append(ref[:n]); tgts.append(tgt); lists.append(STEP_ANGLES[: 60 + n % 7]); centres.append((0.0, 0.0))
    batch = mm.Batch(refs, tgts, lists, centres)
    out, stats = _bounded(engine, matrix, lambda: engine.best_rotation_batch(batch, precision=mm.MM_PRECISION_F32_BOUNDED))
    assert stats["offered"] == sum(len(x) for x in lists), stats
    for p in range(len(refs)):
        oc = oracle.costs_over_angles(refs[p], tgts[p], lists[p], 0.0, 0.0)
        w = int(np.argmin(oc))
        assert out["best_idx"][p] == w and out["best_angle"][p] == lists[p][w] and out["best_cost"][p] == oc[w], (p, w)
