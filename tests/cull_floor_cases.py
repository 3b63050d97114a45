"""The culled screen's value floor restated in numpy, and the directed cases of tests/test_cull_floor_rule.py (CPU) and
tests/test_gpu_screen_cull_floor.py (device).  Not a test module.

The rule (the header of k_screen_mx_cull): P is a candidate's phase-1 mask, u_r / v_c its row and column minima
over P, Tr_I / Tc_J the smallest thr of a row tile / column tile outside P.  A row is SETTLED if u_r <= Tr_I (its minimum
is the full one already), the floor L is the largest settled minimum (0 without one), a row or column is LIVE if its minimum
lies above L, and phase 2 computes a tile outside P unless thr >= max(U'_I, V'_J), the largest live minima of its row tile
and its column tile ("none" below every thr).  The value is the largest minimum as they stand after phase 2."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import model_cull_tiles as model  # noqa: E402

F = np.float32


class Candidate:
    """What the rule did with one candidate (value, brute: the rule's value and the largest full minimum, both from the same
    f64 squared distances; p1, p2: the masks; u, v: minima after phase 1; fu, fv: after phase 2; L; settled rows / columns)."""


def tile_mask(m):
    return np.repeat(np.repeat(m, 32, axis=0), 32, axis=1)


def candidate(d2, thr, p1, floor, lower=None):
    """The rule on one candidate: d2[nrt * 32, nct * 32] f64 squared distances of the slots, thr[nrt, nct], phase-1 mask p1.
    lower: thresholds to use instead of thr for Tr / Tc and the phase-2 rule (a lower threshold is a valid bound too)."""
    nrt, nct = thr.shape
    t = thr if lower is None else lower
    c = Candidate()
    big = np.where(tile_mask(p1), d2, np.inf)
    c.u, c.v = big.min(axis=1), big.min(axis=0)
    out = np.where(p1, np.inf, t)
    c.tr, c.tc = out.min(axis=1), out.min(axis=0)
    c.srow, c.scol = c.u <= np.repeat(c.tr, 32), c.v <= np.repeat(c.tc, 32)
    if floor:
        U, V, c.L = model.floor_maxima(c.u, c.v, t, p1)
        # (the model's L, said again: the largest settled minimum, 0 without one)
        assert c.L == max(0.0, c.u[c.srow].max(initial=0.0), c.v[c.scol].max(initial=0.0))
    else:
        U, V, c.L = c.u.reshape(nrt, 32).max(axis=1), c.v.reshape(nct, 32).max(axis=1), None
    c.p1 = p1
    c.p2 = ~p1 & ~((t > 0) & (t >= np.maximum(U[:, None], V[None, :])))
    big = np.where(tile_mask(p1 | c.p2), d2, np.inf)
    c.fu, c.fv = big.min(axis=1), big.min(axis=0)
    c.value = max(c.fu.max(), c.fv.max(), 0.0)
    c.brute = max(d2.min(axis=1).max(), d2.min(axis=0).max(), 0.0)
    return c


def slots(ref, tgt, mains=(0, 0)):
    """(scaled f64 slot coordinates of the reference and the unrotated target, row circles, column circles, e2s) as
    tools/model_cull_tiles.py lays the sets out (mains: the first run of a set of two, as split_main takes it)."""
    e, e2 = model.scale_and_e2(ref, tgt)
    S = 2.0 ** e
    nrt, nct = (len(ref) + 31) // 32, (len(tgt) + 31) // 32
    ri = model.slot_map(len(ref), model.split_main(len(ref), mains[0]), nrt * 32)
    ci = model.slot_map(len(tgt), model.split_main(len(tgt), mains[1]), nct * 32)
    r32, t32 = ref.astype(F)[ri], tgt.astype(F)[ci]
    rc = model.circles(r32.reshape(nrt, 32, 2), S)
    cc = model.circles(t32.reshape(nct, 32, 2), S)
    e2s = float(F(e2 * S * S) * F(1.000003814697265625))
    return S * r32.astype(np.float64), S * t32.astype(np.float64), rc, cc, e2s


def rotated(b0, c, s):
    cd, sd = np.float64(c), np.float64(s)
    return np.stack([b0[:, 0] * cd - b0[:, 1] * sd, b0[:, 0] * sd + b0[:, 1] * cd], axis=1)


def screen(ref, tgt, angles, group=1, carry=True, floor=True, mains=(0, 0)):
    """The rule over a candidate list in groups of `group` (carry: the leader hands its phase-2 tiles on): [Candidate]."""
    a, b0, rc, cc, e2s = slots(ref, tgt, mains)
    cs = np.stack([np.cos(angles).astype(F), np.sin(angles).astype(F)], axis=1)
    out = []
    for k in range(len(angles)):
        if k % group == 0:
            thr = model.thresholds(rc, model.group_circles(cc, cs[k:k + group]), cs[k, 0], cs[k, 1], e2s, rotated=True)
            m1 = model.phase1(thr)
            lead = None
        b = rotated(b0, cs[k, 0], cs[k, 1])
        d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2)
        c = candidate(d2, thr, m1 | lead if lead is not None and carry else m1, floor)
        c.thr, c.d2 = thr, d2
        if k % group == 0:
            lead = c.p2
        out.append(c)
    return out


# ---- the sets ----
def lumen(n, r=2.3, phase=0.0, squash=0.8):
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    rr = r * (1 + 0.08 * np.sin(3 * t + phase) + 0.04 * np.cos(5 * t - phase))
    return np.stack([rr * np.cos(t), squash * rr * np.sin(t)], axis=1)


def catheter(n, at=(0.1, -0.05)):
    u = np.linspace(0, 2 * np.pi, n, endpoint=False) + 0.3
    return np.stack([at[0] + 0.5 * np.cos(u), at[1] + 0.5 * np.sin(u)], axis=1)


def contour_set(lum, cath, r=2.3, phase=0.0, at=(0.1, -0.05)):
    return np.concatenate([lumen(lum, r, phase), catheter(cath, at)])


def ring(n, r, start=0.0):
    t = start + np.linspace(0, 2 * np.pi, n, endpoint=False)
    return np.stack([r * np.cos(t), r * np.sin(t)], axis=1)


def grid(p, bits=6):
    """Coordinates on the binary grid 2^-bits: exact in f32, their differences and squares exact in f64."""
    return np.round(p * 2.0 ** bits) / 2.0 ** bits


REF3, TGT17 = contour_set(76, 20), contour_set(501, 20, r=2.35, phase=0.7, at=(-0.05, 0.1))      # 96 and 521 points
SET17 = contour_set(501, 20)


def case_outlier():
    """(a) a reference of three row tiles whose last tile is a short arc far outside the target: no column tile is close to
    it, so phase 1 gives it its circle-nearest column tile only, and the rows of the arc's far end have their nearest
    partner in a neighbouring column tile: they are live, made exact in phase 2, and one of them is the value."""
    t = np.radians(np.linspace(-14.0, 14.0, 32))
    arc = np.stack([4.6 * np.cos(t), 4.6 * np.sin(t)], axis=1)
    return np.concatenate([lumen(64), arc]), TGT17, (0, 501), np.radians([0.0, 0.5, 1.0, 1.5, 2.0, 2.5, 3.0, 3.5, 4.0])


def case_column_floor():
    """(b) the roles swapped: a target whose last full tile is such an arc, far outside the reference; the floor comes from a
    settled column of it."""
    t = np.radians(np.linspace(-6.0, 6.0, 32))
    arc = np.stack([3.4 * np.cos(t), 3.4 * np.sin(t)], axis=1)
    tgt = np.concatenate([lumen(489, 2.35, 0.7), arc])
    return contour_set(76, 20), tgt, (76, 0), np.radians(-2.0 + 0.5 * np.arange(9))


def case_nothing_settled():
    """(c) a small ring inside a large one: every row tile and column tile has tiles outside phase 1 whose (loose) thr lies
    below its minima, none is settled and L = 0."""
    return ring(96, 0.5), ring(521, 3.0, 0.01), (0, 0), np.radians(-2.0 + 0.5 * np.arange(9))


def case_all_settled():
    """(d) the target is the reference's contour again, slightly turned: phase 1 holds every tile near a minimum."""
    return SET17, contour_set(501, 20, phase=0.002), (501, 501), np.radians(-1.0 + 0.25 * np.arange(9))


def case_ties():
    """(e) concentric rings on a binary grid, unrotated (cos = 1, sin = 0: every squared distance is exact in f64): the
    points come in orbits of four with one minimum bit for bit, the tiles do not, so rows and columns that are not settled
    have minima EQUAL to the floor a settled one of their orbit gave (u_r == L: not live)."""
    ref = grid(ring(96, 1.0), 4)
    t = grid(ring(520, 2.5), 4)                  # (fourfold symmetric on the grid; the tiles of 32 are not)
    tgt = np.concatenate([t, t[:1]])
    return ref, tgt, (0, 0), np.radians([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0])


def case_far_group():
    """(f) rotations 20 degrees apart in one group."""
    return REF3, TGT17, (76, 501), np.radians(-170.0 + 20.0 * np.arange(18))
