#!/usr/bin/env python3
"""Write tests/golden/bspline/*.npz: the closed B-spline fits of scipy (the reference's recipe,
multimodars/ccta/discretization_map.py:16-83: ``splprep(s, k, per=True, full_output=True)`` then ``splev`` at
``linspace(0, 1, m, endpoint=False)``) on small contours.  Needs scipy; the tests that read the files do not.

A case is kept only if scipy itself is stable on it: the knot vector is unchanged (same length, positions within
1e-9) when s is scaled by 1 +- 1e-3 and when the input is perturbed by 1e-12 relative, and the output is finite.  An
unstable case is replaced by the same contour at a neighbouring s.  Per kept case the file records how far scipy's own output moves under those
perturbations (relative to the contour's bounding-box diagonal).

One file per degree (cases ``c000``, ``c001``, ...): ``<case>_in`` (m, 3), ``<case>_t`` knots, ``<case>_out`` (m, 3),
``<case>_meta`` = [m, k, s, fp, ier, self_sensitivity]; ``names`` lists the cases, ``labels`` what each is.
"""
import os
import sys
import warnings

import numpy as np
from scipy.interpolate import splev, splprep

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "golden", "bspline")
SIZES = (6, 7, 16, 63, 64, 65, 100, 200)
DEGREES = (1, 2, 3, 5)


def contour(m, seed=None, noise=0.05):
    """a noisy lobed ellipse of radius about 2 mm, off the origin"""
    rng = np.random.default_rng(m if seed is None else seed)
    th = np.linspace(0, 2 * np.pi, m, endpoint=False)
    r = 2.0 * (1 + 0.15 * np.cos(3 * th)) + noise * rng.normal(size=m)
    return np.stack([1.3 * r * np.cos(th) + 10, r * np.sin(th) - 5,
                     0.3 * np.sin(2 * th) + noise * rng.normal(size=m) + 40], 1)


def scipy_fit(P, s, k):
    """(knots, out, fp, ier) or None when splprep raises"""
    m = P.shape[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            (tck, _), fp, ier, _ = splprep([P[:, 0].copy(), P[:, 1].copy(), P[:, 2].copy()], s=s, k=k, per=True,
                                           full_output=True, quiet=1)
        except Exception:
            return None
    out = np.stack(splev(np.linspace(0.0, 1.0, m, endpoint=False), tck), 1)
    return np.asarray(tck[0]), out, float(fp), int(ier)


def stable(P, s, k):
    """(fit, self-sensitivity) if scipy is stable on the case, else None"""
    base = scipy_fit(P, s, k)
    if base is None or not np.isfinite(base[1]).all():
        return None
    ext = float(np.linalg.norm(P.max(0) - P.min(0)))
    sens = 0.0
    rng = np.random.default_rng(12345)
    variants = [(P, s * (1 + 1e-3)), (P, s * (1 - 1e-3)), (P * (1 + 1e-12 * rng.uniform(-1, 1, P.shape)), s)]
    for Q, sq in variants:
        f = scipy_fit(Q, sq, k)
        if f is None or len(f[0]) != len(base[0]) or f[3] != base[3] or not np.isfinite(f[1]).all():
            return None
        if np.abs(f[0] - base[0]).max() > 1e-9:              # the same knots, not only as many
            return None
        sens = max(sens, float(np.abs(f[1] - base[1]).max()) / ext)
    return base, sens


def cases():
    for k in DEGREES:
        for m in sorted(set((k, k + 1) + SIZES)):
            for s in (0.0, 0.02, 0.0025 * m, float(m), 100.0):
                yield k, f"ellipse m={m}", contour(m), s
        m = 64
        P = contour(m)
        rep = P.copy(); rep[20] = rep[19]
        closed = P.copy(); closed[-1] = closed[0]
        planar = P.copy(); planar[:, 2] = 40.0
        far = P + 1e3
        for label, Q in (("repeated point", rep), ("last equals first", closed), ("planar", planar), ("translated 1e3", far)):
            for s in (0.0, 0.0025 * m):
                yield k, label, Q, s


def main():
    os.makedirs(OUT, exist_ok=True)
    dropped = []
    for k in DEGREES:
        data, names, labels = {}, [], []
        for kk, label, P, s in cases():
            if kk != k:
                continue
            m = P.shape[0]
            name = f"c{len(names):03d}"
            if m < k + 1 or scipy_fit(P, s, k) is None:
                # too short (returned unchanged) or a ValueError of splprep (zero chord): ier 10 stands for "unchanged"
                data[name + "_in"], data[name + "_t"], data[name + "_out"] = P, np.zeros(0), P.copy()
                data[name + "_meta"] = np.array([m, k, s, 0.0, 10 if m >= k + 1 else 11, 0.0])
                names.append(name); labels.append(label)
                continue
            got = None
            for factor in (1.0, 1.1, 0.9, 1.25, 0.8):
                got = stable(P, s * factor, k)
                if got is not None:
                    s = s * factor
                    break
            if got is None:
                dropped.append((k, label, s))
                continue
            (t, out, fp, ier), sens = got
            data[name + "_in"], data[name + "_t"], data[name + "_out"] = P, t, out
            data[name + "_meta"] = np.array([m, k, s, fp, ier, sens])
            names.append(name); labels.append(label)
        data["names"] = np.array(names)
        data["labels"] = np.array(labels)
        path = os.path.join(OUT, f"closed_k{k}.npz")
        np.savez_compressed(path, **data)
        print(f"{path}: {len(names)} cases, {os.path.getsize(path)} bytes")
    for d in dropped:
        print("dropped (scipy unstable at every neighbouring s):", d)
    return 0


if __name__ == "__main__":
    sys.exit(main())
