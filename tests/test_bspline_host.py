"""The closed smoothing B-spline checker (tests/mm_checkers/bspline.py) against scipy's recorded results
(tests/golden/bspline, written by tools/make_bspline_golden.py) -- no GPU, no scipy needed except for the live test.

Tolerances against scipy are measured, not assumed: over all fixtures the checker's largest deviation from scipy's
output points, relative to the contour's bounding-box diagonal, is
    s = 0 : 0.0       (bit-identical on every interpolated fixture)
    s > 0 : 2.44e-11
and the tests allow 8x that (scipy's Fortran may contract to FMA and orders its Givens sums differently): 0 for the
s = 0 fixtures, which are recorded data.  Only the live-scipy test, which may meet another build of scipy, floors the
s = 0 allowance at 1e-13, five ulps of a coordinate of magnitude 1e3 on a 6 mm contour.  scipy's own output moves
by up to 2.4e-4 (same measure) when s changes by 0.1 % or the input by 1e-12: the s > 0 deviation must stay below that.
"""
import functools
import glob
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mm_checkers import bspline as B  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bspline")
MEASURED_S0, MEASURED_S = 0.0, 2.44e-11
TOL_S0 = 8 * MEASURED_S0
TOL_S0_LIVE = max(TOL_S0, 1e-13)
TOL_S = 8 * MEASURED_S


@functools.lru_cache(maxsize=None)
def fixtures():
    """every case of every file, each with the checker's result (computed once per session)"""
    out = []
    files = sorted(glob.glob(os.path.join(GOLDEN, "closed_k*.npz")))
    assert len(files) == 4
    for f in files:
        z = np.load(f)
        for name in z["names"]:
            meta = z[name + "_meta"]
            case = {"id": os.path.basename(f) + ":" + str(name), "in": z[name + "_in"], "t": z[name + "_t"],
                    "out": z[name + "_out"], "m": int(meta[0]), "k": int(meta[1]), "s": float(meta[2]),
                    "fp": float(meta[3]), "ier": int(meta[4]), "sens": float(meta[5])}
            case["res"] = B.fit_closed(case["in"], case["s"], case["k"])
            out.append(case)
    return out


def extent(P):
    return float(np.linalg.norm(P.max(0) - P.min(0)))


def fitted_cases():
    return [c for c in fixtures() if c["ier"] not in (10, 11)]


def test_fixture_set_covers_the_cases():
    fx = fixtures()
    assert {c["k"] for c in fx} == {1, 2, 3, 5}
    for k in (1, 2, 3, 5):
        assert {k, k + 1, 6, 7, 16, 63, 64, 65, 100, 200} <= {c["m"] for c in fx if c["k"] == k}
    statuses = {c["res"]["status"] for c in fx}
    assert {B.FITTED, B.INTERPOLATED, B.COLLAPSED, B.UNCHANGED_SHORT, B.UNCHANGED_ZERO_CHORD} <= statuses


def test_knots_equal_scipys():
    for c in fitted_cases():
        r = c["res"]
        assert r["n_knots"] == len(c["t"]), c["id"]
        assert np.abs(r["knots"] - c["t"]).max() <= 1e-12, c["id"]


def test_status_maps_to_ier():
    for c in fixtures():
        st = c["res"]["status"]
        if c["ier"] == 11:
            assert st == B.UNCHANGED_SHORT, c["id"]
        else:
            assert st == B.status_of_ier(c["ier"]), (c["id"], st, c["ier"])


def test_residual_conditions():
    seen = set()
    for c in fitted_cases():
        r, P, s = c["res"], c["in"], c["s"]
        seen.add(r["status"])
        if r["status"] == B.FITTED:
            assert abs(r["fp"] - s) <= 1e-3 * s, c["id"]
        elif r["status"] == B.INTERPOLATED:
            # the curve passes through the data at the data parameters (the last point replaced by the first)
            Q = P.copy()
            Q[-1] = Q[0]
            u = np.concatenate([[0.0], np.cumsum(np.sqrt((np.diff(Q, axis=0) ** 2).sum(1)))])
            u /= u[-1]
            t, n, k = [0.0] + list(r["knots"]), r["n_knots"], c["k"]
            cf = r["coef"]
            h, hh = [0.0] * (k + 3), [0.0] * (k + 3)
            for i in range(c["m"] - 1):
                l = k + 1
                while not (u[i] < t[l + 1] or l == n - k - 1):
                    l += 1
                B._bspl(t, k, float(u[i]), l, h, hh)
                for d in range(3):
                    v = sum(cf[l - k - 1 + d * n + j] * h[j] for j in range(1, k + 2))
                    assert abs(v - Q[i, d]) <= 1e-10 * extent(P), (c["id"], i, d)
        elif r["status"] == B.COLLAPSED:
            mean = c["in"][:-1].mean(0)                       # the last point gives way to the first
            assert np.abs(r["points"] - mean).max() <= 1e-12 * max(extent(P), 1.0), c["id"]
            assert np.abs(r["points"] - r["points"][0]).max() <= 1e-12 * max(extent(P), 1.0), c["id"]
    assert {B.FITTED, B.INTERPOLATED, B.COLLAPSED} <= seen


def test_points_against_scipy_within_measured_tolerance():
    worst0 = worsts = sens = 0.0
    for c in fitted_cases():
        d = float(np.abs(c["res"]["points"] - c["out"]).max()) / extent(c["in"])
        if c["s"] == 0.0:
            worst0 = max(worst0, d)
        else:
            worsts = max(worsts, d)
            sens = max(sens, c["sens"])
    print(f"largest deviation from scipy: s=0 {worst0:.3e} (tolerance {TOL_S0:.3e}), s>0 {worsts:.3e} "
          f"(tolerance {TOL_S:.3e}); scipy's own sensitivity {sens:.3e}")
    assert worst0 <= TOL_S0
    assert worsts <= TOL_S
    assert worsts <= sens          # else the restatement does not follow FITPACK's iteration


def test_first_point_of_an_interpolated_contour_is_the_first_input_point():
    for c in fitted_cases():
        if c["res"]["status"] == B.INTERPOLATED and c["s"] == 0.0:
            assert np.abs(c["res"]["points"][0] - c["in"][0]).max() <= 1e-10 * extent(c["in"]), c["id"]


def test_live_scipy_on_random_contours():
    interp = pytest.importorskip("scipy.interpolate")
    sys.path.insert(0, os.path.join(os.path.dirname(GOLDEN), "..", "..", "tools"))
    import make_bspline_golden as G
    rng = np.random.default_rng(2024)
    kept, tries = 0, 0
    while kept < 50 and tries < 400:
        tries += 1
        m = int(rng.integers(8, 49))
        k = int(rng.choice([1, 2, 3, 4, 5]))
        s = float(rng.choice([0.0, 0.01, 0.05, 0.3])) * (m / 16.0)
        P = G.contour(m, seed=1000 + tries, noise=0.08)
        got = G.stable(P, s, k)
        if got is None:
            continue
        (t, out, fp, ier), sens = got
        r = B.fit_closed(P, s, k)
        assert r["status"] == B.status_of_ier(ier), (m, k, s)
        assert r["n_knots"] == len(t) and np.abs(r["knots"] - t).max() <= 1e-12, (m, k, s)
        d = float(np.abs(r["points"] - out).max()) / extent(P)
        assert d <= (TOL_S0_LIVE if s == 0.0 else TOL_S), (m, k, s, d)
        kept += 1
    assert kept == 50
    assert interp is not None


@pytest.mark.parametrize("m", [7, 8, 9, 100, 129, 200])
def test_centroid_is_numpys_mean_bit_for_bit(m):
    a = np.random.default_rng(m).normal(size=(m, 3)) * 37.0 + 11.0
    for d in range(3):
        col = np.ascontiguousarray(a[:, d])
        assert B.pairwise_mean(col) == float(np.mean(col))
    r = B.fit_closed(a, 0.0, 3)
    for d in range(3):
        assert r["centroid"][d] == float(np.mean(np.ascontiguousarray(r["points"][:, d])))


def test_unchanged_contours_and_bad_degrees():
    P = np.random.default_rng(3).normal(size=(12, 3))
    r = B.fit_closed(P[:3], 0.1, 3)
    assert r["status"] == B.UNCHANGED_SHORT and np.array_equal(r["points"], P[:3]) and r["n_knots"] == 0
    r = B.fit_closed(np.zeros((0, 3)), 0.1, 3)
    assert r["status"] == B.UNCHANGED_SHORT and r["points"].shape == (0, 3)
    assert B.fit_closed(P[:4], 0.0, 3)["status"] == B.INTERPOLATED          # m == degree + 1 is fitted
    Q = P.copy()
    Q[5] = Q[4]
    r = B.fit_closed(Q, 0.1, 3)
    assert r["status"] == B.UNCHANGED_ZERO_CHORD and np.array_equal(r["points"], Q)
    Q = P.copy()
    Q[7, 1] = np.nan
    r = B.fit_closed(Q, 0.1, 3)
    assert r["status"] == B.UNCHANGED_NONFINITE and np.array_equal(r["points"], Q, equal_nan=True)
    Q[7, 1] = np.inf
    assert B.fit_closed(Q, 0.0, 2)["status"] == B.UNCHANGED_NONFINITE
    # finite coordinates whose squared chord overflows: unchanged, for every s and degree
    for scale in (1e160, 1.7e308):
        Q = P / np.abs(P).max() * scale
        assert np.isfinite(Q).all()
        for s_, k_ in ((0.0, 3), (0.1, 3), (0.0, 2), (1e300, 1), (0.1, 5)):
            r = B.fit_closed(Q, s_, k_)
            assert r["status"] == B.UNCHANGED_NONFINITE and np.array_equal(r["points"], Q), (scale, s_, k_)
    for k in (0, 6, -1):
        with pytest.raises(ValueError):
            B.fit_closed(P, 0.1, k)
    with pytest.raises(ValueError):
        B.fit_closed(P, -1.0, 3)
    with pytest.raises(ValueError):
        B.fit_closed(np.zeros((B.MAX_POINTS + 1, 3)), 0.0, 3)
