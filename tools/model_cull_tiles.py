#!/usr/bin/env python3
"""Tiles the culled matrix-pipe screen (k_screen_mx_cull) computes per candidate, priced on the host (numpy, no GPU).

The kernel's two-phase rule (its header in csrc/mm_kernels.hip) restated: bounding-box circles per tile of 32 slots with
the slacks of csrc/mm_tile_bound.h, the engine's scale exponent and error bound mx_e2, thr(I, J) per tile pair, the phase-1
mask (every tile with thr <= 0, else the nearest partner of a row or column tile) and the phase-2 mask (thr below the
larger of the row tile's and the column tile's largest phase-1 minimum).  The circles and thr are computed in f32 without
the kernel's fused operations and the phase-1 minima are exact f64 squared distances where the kernel has screened ones
(within e2 of them): a tile count from here can differ from the device's by the few tiles whose thr agrees with a minimum
to that error.  It prices a LAYOUT or a BOUND, it does not replace the device counter (mm_engine_screen_tiles).

Layouts (--layout):
    consecutive   slot j holds point min(j, n - 1): tiles of 32 consecutive indices
    split         a set of two runs (main lumen points, then the catheter's): each run starts a tile of its own, padded
                  with its own last point (mm_tile_slot_point), taken where it adds no tile (mm_tile_split_main)
    both          the two side by side (default)

Groups (--group G): G consecutive candidates share one threshold table and one phase-1 mask, built from circles that hold
a column tile under every rotation of the group (mm_tile_group_circle: the middle rotation's centre, the radius widened by
the farthest of the others), and the group's first candidate hands its phase-2 tiles to the others, which run them in
phase 1 (--no-carry prices the shared thresholds alone).  --runs R prices R runs of G candidates spread over the list
instead of all of it.  With groups the last column is the share of the followers (all but a group's first candidate)
whose phase 2 is empty: the ones the kernel lets go after phase 1 on the group test (mm_engine_screen_early counts them).
--items W cuts the list into W work items the way the engine does (item k: candidates [n k / W, n (k + 1) / W)) and groups
inside each item, as the kernel's waves do: the device's counters are matched item layout for item layout.

    python tools/model_cull_tiles.py --frames 12 --points 501 --pairs 1 2 3 4 --rotations 91
    python tools/model_cull_tiles.py --layout split --rotations 721 --group 8 --runs 15
    python tools/model_cull_tiles.py --layout split --rotations 721 --group 8 --items 23
    python tools/model_cull_tiles.py --layout split --rotations 721 --group 8 --runs 15 --floor

--floor prices the value floor (ScreenOptions::screen_floor): a candidate's value is the MAXIMUM of its minima, so a row or
column whose phase-1 minimum lies at or below a minimum that is already exact cannot raise it and takes no phase-2 tile.
"""
import argparse
import os
import sys

import numpy as np

U = 2.0 ** -24
F = np.float32


def slot_map(n, main, slots):
    """mm_tile_slot_point for j < slots."""
    j = np.arange(slots)
    if main <= 0 or main >= n:
        return np.minimum(j, n - 1)
    edge = (main + 31) // 32 * 32
    return np.where(j < edge, np.minimum(j, main - 1), main + np.minimum(j - edge, n - main - 1))


def split_main(n, main):
    """mm_tile_split_main: the split is taken where it adds no tile."""
    if main <= 0 or main >= n:
        return 0
    return main if (main + 31) // 32 + (n - main + 31) // 32 == (n + 31) // 32 else 0


def scale_and_e2(ref, tgt):
    """The engine's scale exponent and mx_e2 for sets around the rotation centre (0, 0)."""
    r32, t32 = ref.astype(F).astype(np.float64), tgt.astype(F).astype(np.float64)
    ra, rb = np.hypot(r32[:, 0], r32[:, 1]).max(), np.hypot(t32[:, 0], t32[:, 1]).max()
    e = 9 - int(np.frexp(max(ra, rb) * (1.0 + 1e-6))[1])
    R = ra + rb
    return e, U * (47 * R * R + 6 * ra * ra + 27 * rb * rb)


def circles(p, S):
    """mm_tile_circle of every tile: p[tiles, 32, 2] f32 points (unscaled) -> (cx, cy, r) f32."""
    q = F(S) * p
    lo, hi = q.min(axis=1), q.max(axis=1)
    c = F(0.5) * (lo + hi)
    d = q - c[:, None, :]
    m = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]).max(axis=1)
    r = np.sqrt(m) * F(1.000003814697265625) + F(0.0009765625)
    return c[:, 0], c[:, 1], r.astype(F)


def group_circles(cc, cs):
    """mm_tile_group_circle of every column tile for the rotations cs[n, 2] (f32 cos, sin): (cx, cy, r) f32, centres rotated."""
    n = len(cs)
    bx = cc[0][None, :] * cs[:, 0:1] - cc[1][None, :] * cs[:, 1:2]
    by = cc[0][None, :] * cs[:, 1:2] + cc[1][None, :] * cs[:, 0:1]
    mx, my = bx[n // 2], by[n // 2]
    if n == 1:
        return mx, my, cc[2]
    dx, dy = bx - mx[None, :], by - my[None, :]
    m = (dx * dx + dy * dy).max(axis=0)
    return mx, my, (cc[2] + (np.sqrt(m) * F(1.000003814697265625) + F(0.0009765625))).astype(F)


def thresholds(rc, cc, c, s, e2s, rotated=False):
    """thr[nrt, nct] (mm_tile_gap, mm_tile_threshold); the column centres rotated by the f32 (c, s), or taken as they are."""
    bx = cc[0] if rotated else cc[0] * c - cc[1] * s
    by = cc[1] if rotated else cc[0] * s + cc[1] * c
    dx, dy = rc[0][:, None] - bx[None, :], rc[1][:, None] - by[None, :]
    d = np.sqrt(dx * dx + dy * dy)
    gap = d * F(0.999996185302734375) - (rc[2][:, None] + cc[2][None, :]) - F(0.0078125)
    thr = gap * gap * F(0.99999237060546875) - F(e2s)
    return np.where(gap > 0, thr, F(-1.0)).astype(np.float64)


def phase1(thr):
    close = ~(thr > 0)
    m1 = close.copy()
    for i in np.nonzero(~close.any(axis=1))[0]:
        m1[i, np.argmin(thr[i])] = True
    for j in np.nonzero(~close.any(axis=0))[0]:
        m1[np.argmin(thr[:, j]), j] = True
    return m1


def floor_maxima(u, v, thr, m1):
    """The value floor (--floor; the kernel's header): u[nrt * 32], v[nct * 32] the row and column minima after
    phase 1 over the mask m1.  A row is SETTLED if u_r <= Tr_I, the smallest thr of its row tile outside m1 (inf where
    nothing is outside): its minimum is already the full one.  The floor L is the largest settled minimum, rows and columns
    (0 without one), a row is LIVE if u_r > L (a settled one never is).  Returns (U', V', L): the largest live minimum of
    every row tile and column tile, -inf where a tile has none (below every thr)."""
    nrt, nct = thr.shape
    out = np.where(m1, np.inf, thr)
    tr, tc = np.repeat(out.min(axis=1), 32), np.repeat(out.min(axis=0), 32)
    L = max(0.0, u[u <= tr].max(initial=0.0), v[v <= tc].max(initial=0.0))
    ul = np.where(u > L, u, -np.inf).reshape(nrt, 32).max(axis=1)
    vl = np.where(v > L, v, -np.inf).reshape(nct, 32).max(axis=1)
    return ul, vl, L


def count_tiles(ref, tgt, angles, ref_main=0, tgt_main=0, group=1, carry=True, floor=False):
    """(phase-1 tiles, phase-2 tiles) per candidate and row tile, int arrays [len(angles), nrt], for sets around (0, 0)
    laid out as asked (ref_main / tgt_main as the engine would take them: pass them through split_main first).  group > 1:
    the candidates [q group, (q + 1) group) of `angles` share thresholds and phase-1 mask, and with `carry` the first one's
    phase-2 tiles are phase-1 tiles of the others.  floor: phase 2 by the largest LIVE minima (floor_maxima)."""
    e, e2 = scale_and_e2(ref, tgt)
    S = 2.0 ** e
    nrt, nct = (len(ref) + 31) // 32, (len(tgt) + 31) // 32
    ri, ci = slot_map(len(ref), ref_main, nrt * 32), slot_map(len(tgt), tgt_main, nct * 32)
    r32, t32 = ref.astype(F)[ri], tgt.astype(F)[ci]
    rc = circles(r32.reshape(nrt, 32, 2), S)
    cc = circles(t32.reshape(nct, 32, 2), S)
    e2s = float(F(e2 * S * S) * F(1.000003814697265625))
    a = S * r32.astype(np.float64)
    b0 = S * t32.astype(np.float64)
    p1 = np.zeros((len(angles), nrt), dtype=np.int64)
    p2 = np.zeros((len(angles), nrt), dtype=np.int64)
    cs = np.stack([np.cos(angles).astype(F), np.sin(angles).astype(F)], axis=1)
    lead = None
    for k, ang in enumerate(angles):
        c, s = cs[k]
        if k % group == 0:
            thr = thresholds(rc, group_circles(cc, cs[k:k + group]), c, s, e2s, rotated=True)
            m1g = phase1(thr)
            lead = None
        m1 = m1g | lead if lead is not None and carry else m1g
        cd, sd = np.float64(c), np.float64(s)
        b = np.stack([b0[:, 0] * cd - b0[:, 1] * sd, b0[:, 0] * sd + b0[:, 1] * cd], axis=1)
        d2 = ((a[:, None, :] - b[None, :, :]) ** 2).sum(axis=2)
        big = np.where(np.repeat(np.repeat(m1, 32, axis=0), 32, axis=1), d2, np.inf)
        if floor:
            u, v, _ = floor_maxima(big.min(axis=1), big.min(axis=0), thr, m1)
        else:
            u = big.min(axis=1).reshape(nrt, 32).max(axis=1)
            v = big.min(axis=0).reshape(nct, 32).max(axis=1)
        m2 = ~m1 & ~((thr > 0) & (thr >= np.maximum(u[:, None], v[None, :])))
        if k % group == 0:
            lead = m2
        p1[k], p2[k] = m1.sum(axis=1), m2.sum(axis=1)
    return p1, p2


def search_sets(g, sample):
    """The within-pullback search sets of a FlatGeometry (align_within.rs:173-191: downsample(lumen, sample) ++
    downsample(catheter, ceil(n_cath * sample / len_lumen0))), each centred on its frame's centroid: [(points, main)]."""
    def down(p, n):
        if len(p) <= n:
            return p
        return p[(np.arange(n) * (len(p) / n)).astype(np.int64)]
    len0 = int(g.lumen_off[1] - g.lumen_off[0])
    has_c = g.cath_off is not None and len(g.cath_off) > 1
    take_c = int(np.ceil(int(g.cath_off[1] - g.cath_off[0]) * (sample / len0))) if has_c else 0
    out = []
    for i in range(g.n_frames):
        lum = down(g.lumen[g.lumen_off[i]:g.lumen_off[i + 1], :2], sample)
        cath = down(g.cath[g.cath_off[i]:g.cath_off[i + 1], :2], take_c) if take_c > 0 else np.zeros((0, 2))
        pts = np.concatenate([lum, cath]) - g.centroids[i, :2]
        out.append((pts, len(lum) if len(cath) and len(lum) else 0))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--points", type=int, default=501, help="points per lumen contour and sample size")
    ap.add_argument("--pairs", type=int, nargs="+", default=[1, 2, 3, 4], help="frame pairs (i - 1, i)")
    ap.add_argument("--rotations", type=int, default=91, help="candidates over +-180 degrees")
    ap.add_argument("--layout", choices=("consecutive", "split", "both"), default="both")
    ap.add_argument("--group", type=int, default=1, help="candidates that share thresholds and phase-1 mask")
    ap.add_argument("--no-carry", action="store_true", help="the first candidate's phase-2 tiles are not handed on")
    ap.add_argument("--floor", action="store_true", help="phase 2 by the value floor: only rows and columns that can still raise the value")
    ap.add_argument("--items", type=int, default=1, help="work items the list is cut into; groups start anew in each")
    ap.add_argument("--runs", type=int, default=0, help="price this many runs of --group candidates spread over the list (0: all)")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from multimoda_rs_amd.synth import synthetic_pullback
    sets = search_sets(synthetic_pullback(a.frames, a.points), a.points)
    angles = np.radians(np.linspace(-180.0, 180.0, a.rotations))
    if a.runs > 0:
        starts = np.linspace(0, max(0, len(angles) - a.group), a.runs).astype(np.int64)
        angles = np.concatenate([angles[i:i + a.group] for i in starts])
    layouts = ("consecutive", "split") if a.layout == "both" else (a.layout,)
    print("layout        pair  tiles/candidate  phase 1   rows2   per row tile (phase 1 + 2)" + ("   followers: empty phase 2" if a.group > 1 else ""))
    for lay in layouts:
        tot, tot1, rows, rows2, early = [], [], [], [], []
        for i in a.pairs:
            (ref, rm), (tgt, tm) = sets[i - 1], sets[i]
            if lay == "consecutive":
                rm = tm = 0
            n, nw = len(angles), max(1, a.items)
            cuts = [(n * k // nw, n * (k + 1) // nw) for k in range(nw)]
            parts = [count_tiles(ref, tgt, angles[a0:a1], split_main(len(ref), rm), split_main(len(tgt), tm), a.group, not a.no_carry, a.floor)
                     for a0, a1 in cuts if a1 > a0]
            p1, p2 = (np.concatenate([q[h] for q in parts]) for h in (0, 1))
            per_row = (p1 + p2).mean(axis=0)
            tot.append(per_row.sum()); tot1.append(p1.sum(axis=1).mean()); rows.append(per_row)
            rows2.append((p2 > 0).sum(axis=1).mean())
            share = ""
            if a.group > 1:
                fol = np.concatenate([np.arange(a1 - a0) % a.group != 0 for a0, a1 in cuts if a1 > a0])
                early.append((fol & (p2.sum(axis=1) == 0)).sum() / max(1, fol.sum()))
                share = "   %d of %d = %.3f" % ((fol & (p2.sum(axis=1) == 0)).sum(), fol.sum(), early[-1])
            print("%-12s  %4d  %15.1f  %7.1f  %6.1f   %s%s" % (lay, i, tot[-1], tot1[-1], rows2[-1], " ".join("%.1f" % x for x in per_row), share))
        print("%-12s  mean  %15.1f  %7.1f  %6.1f   %s%s" % (lay, np.mean(tot), np.mean(tot1), np.mean(rows2),
                                                            " ".join("%.1f" % x for x in np.mean(rows, axis=0)),
                                                            "   %.3f" % np.mean(early) if early else ""))


if __name__ == "__main__":
    main()
