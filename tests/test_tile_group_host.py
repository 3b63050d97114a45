"""The culled screen's GROUP bound (mm_tile_group_circle, csrc/mm_tile_bound.h), checked on the host against f64.

With WorkItem::pad = G > 1 a wave of k_screen_mx_cull builds one threshold table for G consecutive candidates, from one
circle per column tile that must hold the tile under EVERY rotation of the group.  The screened values stay bit-identical
only if that table is a lower bound for each candidate of the group: thr(I, J) <= (exact squared distance) - e2 for every
point pair of tile (I, J) under every rotation.  mm_tile_bound_probe_group runs the kernel's own f32 code on the host; here
each group is rotated in f32 with the kernel's fused form (and exactly, by the same f32 cos / sin) and compared in f64:
  * every point of every candidate's column tile lies inside the widened circle (a group of one is not widened: there the
    rotation's 2^-11, which mm_tile_gap carries, is allowed);
  * thr is at most the smallest exact squared distance of the tile pair over the group, less e2 in scaled units.
Nothing in the proof assumes close, ordered or distinct angles: the groups below include far, shuffled and repeated ones.
A group of one must reproduce mm_tile_bound_probe_split bit for bit, and the staging rule (mm_screen_group_auto) is pinned."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from mx_worst_cases import on_ties  # noqa: E402

U = 2.0 ** -24
P = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731


@pytest.fixture(scope="module")
def native():
    import __graft_entry__ as ge
    ge.build()
    import multimoda_rs_amd as mm
    return mm._native


def _f32_fma(a, b, c):
    """f32 fma(a, b, c) for f32 inputs (tests/test_tile_bound_host.py)."""
    return (a.astype(np.float64) * np.float64(b) + c.astype(np.float64)).astype(np.float32)


def _scale(ref32, tgt32):
    ra = np.hypot(ref32[:, 0].astype(np.float64), ref32[:, 1].astype(np.float64)).max()
    rb = np.hypot(tgt32[:, 0].astype(np.float64), tgt32[:, 1].astype(np.float64)).max()
    e = 9 - int(np.frexp(max(ra, rb) * (1.0 + 1e-6))[1])
    R = ra + rb
    return e, U * (47 * R * R + 6 * ra * ra + 27 * rb * rb)


def _slots(native, n, main):
    out = np.zeros(32 * ((n + 31) // 32), dtype=np.int32)
    assert native.lib().mm_tile_slot_map(int(n), int(main), len(out), P(out)) >= 0
    return out


def _xy(p):
    return (np.ascontiguousarray(p[:, k], dtype=np.float32) for k in (0, 1))


def _probe_group(native, ref32, tgt32, mains, e, cs, e2):
    rx, ry = _xy(ref32)
    tx, ty = _xy(tgt32)
    nrt, nct = (len(rx) + 31) // 32, (len(tx) + 31) // 32
    circ = np.zeros(4 * (nrt + nct), dtype=np.float32)
    thr = np.zeros(nrt * nct, dtype=np.float32)
    cs = np.ascontiguousarray(cs, dtype=np.float32)
    rc = native.lib().mm_tile_bound_probe_group(P(rx), P(ry), len(rx), P(tx), P(ty), len(tx), int(mains[0]), int(mains[1]),
                                                int(e), P(cs), len(cs), float(e2), P(circ), P(thr))
    assert rc == 0, native.last_error()
    return circ.reshape(-1, 4), thr.reshape(nrt, nct)


def _check_group(native, ref, tgt, angles, mains=(0, 0)):
    """One group of rotations: containment and thr <= low for every candidate.  Returns the tile pairs with a threshold."""
    ref32, tgt32 = ref.astype(np.float32), tgt.astype(np.float32)
    e, e2 = _scale(ref32, tgt32)
    S = np.float32(2.0 ** e)
    e2s = e2 * 2.0 ** (2 * e)
    cs = np.stack([np.cos(angles).astype(np.float32), np.sin(angles).astype(np.float32)], axis=1)
    circ, thr = _probe_group(native, ref32, tgt32, mains, e, cs, e2)
    nrt, nct = thr.shape
    ri, ci = _slots(native, len(ref32), mains[0]), _slots(native, len(tgt32), mains[1])
    ax, ay = (S * ref32[ri, 0]).astype(np.float64), (S * ref32[ri, 1]).astype(np.float64)
    bx, by = S * tgt32[ci, 0], S * tgt32[ci, 1]                           # f32, as the kernel holds them
    ccx, ccy, ccr = (np.repeat(circ[nrt:, k].astype(np.float64), 32) for k in (0, 1, 2))
    slack = 2.0 ** -11 if len(angles) == 1 else 0.0
    low = np.full((nrt, nct), np.inf)
    for c, s in cs:
        ex = bx.astype(np.float64) * np.float64(c) - by.astype(np.float64) * np.float64(s)
        ey = bx.astype(np.float64) * np.float64(s) + by.astype(np.float64) * np.float64(c)
        kx = _f32_fma(bx, c, -(by * s)).astype(np.float64)
        ky = _f32_fma(bx, s, by * c).astype(np.float64)
        for px, py in ((ex, ey), (kx, ky)):
            assert (np.hypot(px - ccx, py - ccy) <= ccr + slack).all(), (angles, c, s)
            d2 = (ax[:, None] - px[None, :]) ** 2 + (ay[:, None] - py[None, :]) ** 2
            low = np.minimum(low, d2.reshape(nrt, 32, nct, 32).min(axis=(1, 3)))
    has = thr > 0
    bad = has & ~(thr.astype(np.float64) <= low - e2s)
    assert not bad.any(), (angles, np.argwhere(bad)[:4], thr[bad][:4], (low - e2s)[bad][:4])
    return int(has.sum())


def _contour(rng, n, r, wobble=0.1):
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    rr = r * (1 + wobble * np.sin(3 * t + rng.uniform(0, 6)))
    return np.stack([rr * np.cos(t), rr * np.sin(t)], axis=1)


def _groups():
    """(name, angles in radians) of the groups every set pair is probed with."""
    rng = np.random.default_rng(8)
    out = []
    for base in (-180.0, -33.25, 0.0, 176.5):
        out.append(("8 x 0.5 deg from %g" % base, np.radians(base + 0.5 * np.arange(8))))
    out.append(("8 x 20 deg", np.radians(-70.0 + 20.0 * np.arange(8))))
    out.append(("shuffled", np.radians(rng.permutation(np.linspace(-180.0, 180.0, 8, endpoint=False)))))
    out.append(("180 deg jump", np.radians([10.0, 10.5, 11.0, 11.5, 190.0, 190.5, 191.0, 191.5])))
    out.append(("repeated", np.radians([30.0] * 4 + [30.5] * 3 + [30.0])))
    out.append(("all equal", np.radians([-12.5] * 8)))
    out.append(("single", np.radians([77.0])))
    out.append(("two", np.radians([77.0, 77.5])))
    out.append(("seven", np.radians(1.0 + 0.5 * np.arange(7))))
    return out


def _set_pairs():
    rng = np.random.default_rng(41)
    pairs = [("contours 521", _contour(rng, 521, 2.0), _contour(rng, 521, 2.1), (0, 0)),
             ("contours 521, split 501", _contour(rng, 521, 2.0), _contour(rng, 521, 2.1), (501, 501)),
             ("3 x 17 tiles", _contour(rng, 73, 2.0), _contour(rng, 521, 2.1), (53, 501))]
    # the radii and tie coordinates of the directed error search (tests/mx_worst_cases.py)
    for rmax in (511.9, 300.0, 256.01):
        for jit in (-1, 0, 1):
            pairs.append(("ties r=%g jitter=%d" % (rmax, jit), on_ties(rng, 544, rmax, jit), on_ties(rng, 544, rmax, jit), (0, 0)))
    small = rng.normal(0, 2.0 ** -9, (544, 2))
    far = small.copy(); far[0] = (500.0, -100.0)
    pairs += [("outlier in ref", far, small + 2.0 ** -11, (0, 0)), ("outlier in tgt", small + 2.0 ** -11, far, (0, 0))]
    return pairs


SETS = _set_pairs()


@pytest.mark.parametrize("k", range(len(SETS)), ids=[s[0] for s in SETS])
def test_group_bound_holds_for_every_candidate(native, k):
    name, ref, tgt, mains = SETS[k]
    skipped = {g: _check_group(native, ref, tgt, ang, mains) for g, ang in _groups()}
    if name == "contours 521":
        # the bound is worth something where it is meant to be used, and worth less for far rotations
        assert skipped["8 x 0.5 deg from 0"] > 150 and skipped["single"] > skipped["8 x 0.5 deg from 0"] >= skipped["8 x 20 deg"]


@pytest.mark.parametrize("scale", [2.0 ** -7, 3.0e4, 1e-20, 1e20])
def test_group_bound_at_other_scales(native, scale):
    rng = np.random.default_rng(5)
    a, b = _contour(rng, 521, 2.0) * scale, on_ties(rng, 544, 511.9, 0) * scale
    for _, ang in _groups()[3:8]:
        _check_group(native, a, b, ang)
        _check_group(native, b, a, ang)


def test_a_group_of_one_is_the_rule_per_candidate(native):
    """n == 1: circles and thr of mm_tile_bound_probe_split, bit for bit, with and without the split layout."""
    rng = np.random.default_rng(2)
    for ref, tgt, mains in ((_contour(rng, 521, 2.0), _contour(rng, 521, 2.1), (501, 501)),
                            (on_ties(rng, 544, 511.9, 0), on_ties(rng, 97, 300.0, 1), (0, 60))):
        ref32, tgt32 = ref.astype(np.float32), tgt.astype(np.float32)
        e, e2 = _scale(ref32, tgt32)
        rx, ry = _xy(ref32)
        tx, ty = _xy(tgt32)
        for ang in np.radians([0.0, 0.5, 33.0, -179.5, 90.0]):
            c, s = np.float32(np.cos(ang)), np.float32(np.sin(ang))
            circ, thr = _probe_group(native, ref32, tgt32, mains, e, [[c, s]], e2)
            circ1, thr1 = np.zeros(circ.size, dtype=np.float32), np.zeros(thr.size, dtype=np.float32)
            rc = native.lib().mm_tile_bound_probe_split(P(rx), P(ry), len(rx), P(tx), P(ty), len(tx), mains[0], mains[1], int(e),
                                                        C.c_float(c), C.c_float(s), float(e2), P(circ1), P(thr1))
            assert rc == 0
            assert np.array_equal(circ.ravel().view(np.uint32), circ1.view(np.uint32))
            assert np.array_equal(thr.ravel().view(np.uint32), thr1.view(np.uint32))


def test_bad_groups_are_refused(native):
    z = np.zeros(64, dtype=np.float32)
    out = np.zeros(64, dtype=np.float32)
    cs = np.zeros(2 * 65, dtype=np.float32)
    L = native.lib()
    assert L.mm_tile_bound_probe_group(P(z), P(z), 64, P(z), P(z), 64, 0, 0, 0, P(cs), 0, 0.0, P(out), P(out)) != 0
    assert L.mm_tile_bound_probe_group(P(z), P(z), 64, P(z), P(z), 64, 0, 0, 0, P(cs), 65, 0.0, P(out), P(out)) != 0
    assert L.mm_tile_bound_probe_group(P(z), P(z), 64, P(z), P(z), 64, 0, 0, 0, None, 1, 0.0, P(out), P(out)) != 0


def _auto(native, deg):
    a = np.ascontiguousarray(np.radians(np.asarray(deg, dtype=np.float64)))
    return native.lib().mm_screen_group_auto(P(a), len(a))


def test_staging_rule(native):
    """The largest G <= 8 whose span (G - 1) x the median step is at most 3.5 degrees."""
    assert _auto(native, np.linspace(-180.0, 180.0, 721)) == 8            # 0.5 degrees, the flagship's list
    assert _auto(native, np.linspace(-180.0, 180.0, 181)) == 2            # 2 degrees
    assert _auto(native, np.arange(-1.0, 1.0, 0.01)) == 8
    assert _auto(native, np.arange(-30.0, 30.0, 1.0)) == 4
    assert _auto(native, np.arange(-30.0, 30.0, 0.6)) == 4
    assert _auto(native, np.arange(-30.0, 30.0, 3.5)) == 2
    assert _auto(native, np.arange(-30.0, 30.0, 4.0)) == 1
    # a jump between two ranges does not move the median
    assert _auto(native, np.concatenate([np.arange(-20.0, 0.0, 0.5), np.arange(160.0, 180.0, 0.5)])) == 8
    assert _auto(native, np.concatenate([np.arange(0.0, 10.0, 2.0), np.arange(200.0, 210.0, 2.0)])) == 2
    # descending lists count like ascending ones; a shuffled one has no small typical step
    assert _auto(native, np.linspace(180.0, -180.0, 721)) == 8
    assert _auto(native, np.random.default_rng(0).permutation(np.linspace(-180.0, 180.0, 721))) == 1
    assert _auto(native, [12.0]) == 1
    assert _auto(native, [12.0, 12.5]) == 8
    assert _auto(native, [12.0] * 9) == 8                                 # repeated angles: no span at all
    assert native.lib().mm_screen_group_auto(None, 3) < 0
