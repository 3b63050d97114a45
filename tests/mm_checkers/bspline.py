"""Closed smoothing B-spline contours: the checker of csrc/mm_bspline_fit.h / mm_bspline_kernels.hip.

The algorithm is Dierckx's closed-curve smoothing (P. Dierckx, "Algorithms for smoothing data with periodic and
parametric splines", CGIP 20 (1982); "Curve and surface fitting with splines", OUP 1993, ch. 9), the one behind
``scipy.interpolate.splprep(per=True)`` followed by ``splev`` at ``linspace(0, 1, m, endpoint=False)``, restated here
in plain Python floats (IEEE f64, never fused) -- statement for statement the device's arithmetic order, so the two
agree bit for bit.  Nothing here imports scipy.

Arrays are 1-based like the published algorithm (index 0 is unused): the index guards for tiny systems (fewer interior
knots than border columns) then read exactly as in the book.

Statuses (``mm_bspline_status`` of include/mm_ccta.h): FITTED |fp - s| <= 1e-3 s; INTERPOLATED s = 0 (or the knot set
grew to the interpolation set); COLLAPSED the least-squares constant already has fp0 - s < 1e-3 s;
UNCHANGED_SHORT m < k + 1; UNCHANGED_ZERO_CHORD two consecutive points coincide (after the last point is replaced by
the first); UNCHANGED_NONFINITE; ITERATION_LIMIT the search for p stopped early (20 steps, or a non-monotone F(p)), the
result is used.
"""
from __future__ import annotations

import math

import numpy as np

FITTED, INTERPOLATED, COLLAPSED, UNCHANGED_SHORT, UNCHANGED_ZERO_CHORD, UNCHANGED_NONFINITE, ITERATION_LIMIT = range(7)
STATUS_NAMES = ("fitted", "interpolated", "collapsed", "unchanged_short", "unchanged_zero_chord",
                "unchanged_nonfinite", "iteration_limit")
MAX_POINTS = 256
TOL = 1e-3
MAXIT = 20
IDIM = 3


def status_of_ier(ier: int) -> int:
    """scipy's ``ier`` -> status (10 is the ValueError of a zero chord)."""
    return {0: FITTED, -1: INTERPOLATED, -2: COLLAPSED, 1: ITERATION_LIMIT, 2: ITERATION_LIMIT, 3: ITERATION_LIMIT,
            10: UNCHANGED_ZERO_CHORD}[int(ier)]


def pairwise_mean(a) -> float:
    """np.mean of a contiguous 1-D f64 array: numpy's pairwise sum (8 accumulators, blocks of 128), then / n."""
    a = [float(v) for v in a]

    def psum(lo, n):
        if n < 8:
            r = -0.0
            for i in range(n):
                r = r + a[lo + i]
            return r
        if n <= 128:
            r = a[lo:lo + 8]
            i = 8
            while i < n - (n % 8):
                for j in range(8):
                    r[j] = r[j] + a[lo + i + j]
                i += 8
            res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
            while i < n:
                res = res + a[lo + i]
                i += 1
            return res
        n2 = n // 2
        n2 -= n2 % 8
        return psum(lo, n2) + psum(lo + n2, n - n2)

    n = len(a)
    if n == 0:
        return float("nan")
    return (0.0 + psum(0, n)) / n


def _givens(piv, ww):
    store = abs(piv)
    if store >= ww:
        dd = store * math.sqrt(1.0 + (ww / piv) * (ww / piv))
    else:
        dd = ww * math.sqrt(1.0 + (piv / ww) * (piv / ww))
    return ww / dd, piv / dd, dd          # cos, sin, new ww


def _bspl(t, k, x, l, h, hh):
    """the k + 1 B-splines of degree k that are non-zero on t[l] <= x < t[l + 1], into h[1..k+1]"""
    h[1] = 1.0
    for j in range(1, k + 1):
        for i in range(1, j + 1):
            hh[i] = h[i]
        h[1] = 0.0
        for i in range(1, j + 1):
            li = l + i
            lj = li - j
            if t[li] == t[lj]:
                h[i + 1] = 0.0
            else:
                f = hh[i] / (t[li] - t[lj])
                h[i] = h[i] + f * (t[li] - x)
                h[i + 1] = f * (x - t[lj])


def _back_periodic(a, b, z, zo, n, k, c, co):
    """solve the n x n system | a ' b | c = z: a upper band (k + 1 wide, rows 1..n-k), b the last k columns.
    z and c are read / written from offsets zo / co."""
    n2 = n - k
    l = n
    for i in range(1, k + 1):
        store = z[zo + l]
        j = k + 2 - i
        if i != 1:
            l0 = l
            for l1 in range(j, k + 1):
                l0 += 1
                store = store - c[co + l0] * b[l][l1]
        c[co + l] = store / b[l][j - 1]
        l -= 1
        if l == 0:
            return
    for i in range(1, n2 + 1):
        store = z[zo + i]
        l = n2
        for j in range(1, k + 1):
            l += 1
            store = store - c[co + l] * b[i][j]
        c[co + i] = store
    i = n2
    c[co + i] = c[co + i] / a[i][1]
    if i == 1:
        return
    for j in range(2, n2 + 1):
        i -= 1
        store = c[co + i]
        i1 = k
        if j <= k:
            i1 = j - 1
        l = i
        for l0 in range(1, i1 + 1):
            l += 1
            store = store - c[co + l] * a[i][l0 + 1]
        c[co + i] = store / a[i][1]


def _disc(t, n, k2, b):
    """jumps of the k-th derivative of the B-splines at the interior knots t[k+2..n-k-1], scaled"""
    k1 = k2 - 1
    k = k1 - 1
    nk1 = n - k1
    nrint = nk1 - k
    fac = float(nrint) / (t[nk1 + 1] - t[k1])
    h = [0.0] * (2 * k1 + 2)
    for l in range(k2, nk1 + 1):
        lmk = l - k1
        for j in range(1, k1 + 1):
            ik = j + k1
            lj = l + j
            lk = lj - k2
            h[j] = t[l] - t[lk]
            h[ik] = t[l] - t[lj]
        lp = lmk
        for j in range(1, k2 + 1):
            jk = j
            prod = h[j]
            for _ in range(1, k + 1):
                jk += 1
                prod = prod * h[jk] * fac
            lk = lp + k1
            b[lmk][j] = (t[lk] - t[lp]) / prod
            lp += 1


def _new_knot(u, t, n, fpint, nrdata, nrint):
    """split the knot interval with the largest residual at its middle data point; returns (n + 1, nrint + 1)"""
    k = (n - nrint - 1) // 2
    fpmax = 0.0
    jbegin = 1
    number = maxpt = maxbeg = 0
    for j in range(1, nrint + 1):
        jpoint = nrdata[j]
        if not (fpmax >= fpint[j] or jpoint == 0):
            fpmax = fpint[j]
            number = j
            maxpt = jpoint
            maxbeg = jbegin
        jbegin = jbegin + jpoint + 1
    if number == 0:
        raise ZeroDivisionError("no knot interval can take a knot")      # NaN residuals: treated like a singular system
    ihalf = maxpt // 2 + 1
    nrx = maxbeg + ihalf
    nxt = number + 1
    if nxt <= nrint:
        for j in range(nxt, nrint + 1):
            jj = nxt + nrint - j
            fpint[jj + 1] = fpint[jj]
            nrdata[jj + 1] = nrdata[jj]
            jk = jj + k
            t[jk + 1] = t[jk]
    nrdata[number] = ihalf - 1
    nrdata[nxt] = maxpt - ihalf
    am = float(maxpt)
    an = float(nrdata[number])
    fpint[number] = fpmax * an / am
    an = float(nrdata[nxt])
    fpint[nxt] = fpmax * an / am
    jk = nxt + k
    t[jk] = u[nrx]
    return n + 1, nrint + 1


def _rati(p1, f1, p2, f2, p3, f3):
    """root of the rational interpolant through three (p, F(p) - s) pairs; p3 < 0 stands for infinity.
    Returns (p, p1, f1, p3, f3) with the bracket moved to (p2, f2) on its side."""
    if p3 > 0.0:
        h1 = f1 * (f2 - f3)
        h2 = f2 * (f3 - f1)
        h3 = f3 * (f1 - f2)
        p = -(p1 * p2 * h3 + p2 * p3 * h1 + p3 * p1 * h2) / (p1 * h1 + p2 * h2 + p3 * h3)
    else:
        p = (p1 * (f1 - f3) * f2 - p2 * (f2 - f3) * f1) / ((f1 - f2) * f3)
    if f2 < 0.0:
        return p, p1, f1, p2, f2
    return p, p2, f2, p3, f3


def _closed_curve(x, u, m, k, s):
    """x[1..3m] (xyz interleaved, point m already replaced by point 1), u[1..m] -> (ier, n, t, c, fp, p).
    c holds the three coordinate blocks of n coefficients each."""
    k1, k2 = k + 1, k + 2
    nest = m + 2 * k
    t = [0.0] * (nest + 2)
    fpint = [0.0] * (nest + 2)
    nrdata = [0] * (nest + 2)
    z = [0.0] * (IDIM * nest + 2)
    c = [0.0] * (IDIM * nest + 2)
    a1 = [[0.0] * (k1 + 1) for _ in range(nest + 1)]
    a2 = [[0.0] * (k1 + 1) for _ in range(nest + 1)]
    b = [[0.0] * (k2 + 1) for _ in range(nest + 1)]
    g1 = [[0.0] * (k2 + 1) for _ in range(nest + 1)]
    g2 = [[0.0] * (k2 + 1) for _ in range(nest + 1)]
    q = [[0.0] * (k1 + 1) for _ in range(m + 1)]
    h = [0.0] * (k2 + 2)
    hh = [0.0] * (k2 + 2)
    h1 = [0.0] * (k2 + 2)
    h2 = [0.0] * (k2 + 2)
    xi = [0.0] * (IDIM + 1)

    m1 = m - 1
    kk, kk1 = k, k1
    nmin = 2 * k1
    per = u[m] - u[1]
    acc = TOL * s
    nmax = m + 2 * k
    fp0 = fpold = 0.0
    nplus = 0
    n = nmin

    def interpolation_knots():
        """knots at the data parameters (odd k) or their midpoints (even k); True if the curve is already done"""
        nonlocal kk, kk1
        if k % 2 == 0:
            for i in range(2, m1 + 1):
                t[i + k] = (u[i] + u[i - 1]) * 0.5
            return False
        for i in range(2, m1 + 1):
            t[i + k] = u[i]
        if s > 0.0:
            return False
        kk, kk1 = k - 1, k
        if kk > 0:
            return False
        # degree 1 through every point: the coefficients are the data
        t[1] = t[m] - per
        t[2] = u[1]
        t[m + 1] = u[m]
        t[m + 2] = t[3] + per
        jj = 0
        for i in range(1, m1 + 1):
            j = i
            for _ in range(IDIM):
                jj += 1
                c[j] = x[jj]
                j += n
        jj, j = 1, m
        for _ in range(IDIM):
            c[j] = c[jj]
            j += n
            jj += n
        return True

    if s > 0.0 or nmax == nmin:
        # the least-squares constant and its residual fp0
        d1 = 0.0
        for j in range(1, IDIM + 1):
            z[j] = 0.0
        jj = 0
        for it in range(1, m1 + 1):
            cs, sn, d1 = _givens(1.0, d1)
            for j in range(1, IDIM + 1):
                jj += 1
                fac = 1.0 * x[jj]
                zj = z[j]
                z[j] = cs * zj + sn * fac
                fac = cs * fac - sn * zj
                fp0 = fp0 + fac * fac
        for j in range(1, IDIM + 1):
            z[j] = z[j] / d1
        fpms = fp0 - s
        if fpms < acc or nmax == nmin:
            for i in range(1, k1 + 1):
                t[i] = u[1] - float(k1 - i) * per
                t[i + k1] = u[m] + float(i - 1) * per
            n = nmin
            j1 = 0
            for j in range(1, IDIM + 1):
                for i in range(1, k1 + 1):
                    c[j1 + i] = z[j]
                j1 += n
            return -2, n, t, c, fp0, 0.0
        fpold = fp0
        nplus = 1
        n = nmin + 1
        mm = (m + 1) // 2
        t[k2] = u[mm]
        nrdata[1] = mm - 2
        nrdata[2] = m1 - mm
    else:
        n = nmax
        if interpolation_knots():
            return -1, n, t, c, 0.0, 0.0

    fp = 0.0
    fpms = 0.0
    n7 = n10 = 0
    part2 = False
    while not part2:
        restart = False
        for _iter in range(1, m + 1):
            nrint = n - nmin + 1
            t[k1] = u[1]
            nk1 = n - k1
            nk2 = nk1 + 1
            t[nk2] = u[m]
            for j in range(1, k + 1):
                t[nk2 + j] = t[k1 + j] + per
                t[k1 - j] = t[nk2 - j] - per
            nc = IDIM * n
            for i in range(1, nc + 1):
                z[i] = 0.0
            for i in range(1, nk1 + 1):
                for j in range(1, kk1 + 1):
                    a1[i][j] = 0.0
            n7 = nk1 - k
            n10 = n7 - kk
            jper = 0
            fp = 0.0
            l = k1
            jj = 0
            for it in range(1, m1 + 1):
                ui = u[it]
                for j in range(1, IDIM + 1):
                    jj += 1
                    xi[j] = x[jj]
                while not ui < t[l + 1] and l < nk1:
                    l += 1
                _bspl(t, k, ui, l, h, hh)
                for i in range(1, k1 + 1):
                    q[it][i] = h[i]
                l5 = l - k1
                if l5 < n10:
                    # a row that touches no border column
                    j = l5
                    for i in range(1, kk1 + 1):
                        j += 1
                        piv = h[i]
                        if piv == 0.0:
                            continue
                        cs, sn, a1[j][1] = _givens(piv, a1[j][1])
                        j1 = j
                        for j2 in range(1, IDIM + 1):
                            av, bv = xi[j2], z[j1]
                            z[j1] = cs * bv + sn * av
                            xi[j2] = cs * av - sn * bv
                            j1 += n
                        if i == kk1:
                            break
                        i2 = 1
                        for i1 in range(i + 1, kk1 + 1):
                            i2 += 1
                            av, bv = h[i1], a1[j][i2]
                            a1[j][i2] = cs * bv + sn * av
                            h[i1] = cs * av - sn * bv
                    for j2 in range(1, IDIM + 1):
                        fp = fp + xi[j2] * xi[j2]
                    continue
                if jper == 0:
                    for i in range(1, n7 + 1):
                        for j in range(1, kk + 1):
                            a2[i][j] = 0.0
                    jk = n10 + 1
                    for i in range(1, kk + 1):
                        ik = jk
                        for j in range(1, kk1 + 1):
                            if ik <= 0:
                                break
                            a2[ik][i] = a1[ik][j]
                            ik -= 1
                        jk += 1
                    jper = 1
                for i in range(1, kk + 1):
                    h1[i] = 0.0
                    h2[i] = 0.0
                h1[kk1] = 0.0
                j = l5 - n10
                for i in range(1, kk1 + 1):
                    j += 1
                    l0 = j
                    while True:
                        l1 = l0 - kk
                        if l1 <= 0:
                            h2[l0] = h2[l0] + h[i]
                            break
                        if l1 <= n10:
                            h1[l1] = h[i]
                            break
                        l0 = l1 - n10
                for j in range(1, n10 + 1):
                    piv = h1[1]
                    if piv == 0.0:
                        for i in range(1, kk + 1):
                            h1[i] = h1[i + 1]
                        h1[kk1] = 0.0
                        continue
                    cs, sn, a1[j][1] = _givens(piv, a1[j][1])
                    j1 = j
                    for j2 in range(1, IDIM + 1):
                        av, bv = xi[j2], z[j1]
                        z[j1] = cs * bv + sn * av
                        xi[j2] = cs * av - sn * bv
                        j1 += n
                    for i in range(1, kk + 1):
                        av, bv = h2[i], a2[j][i]
                        a2[j][i] = cs * bv + sn * av
                        h2[i] = cs * av - sn * bv
                    if j == n10:
                        break
                    i2 = min(n10 - j, kk)
                    i1 = 1
                    for i in range(1, i2 + 1):
                        i1 = i + 1
                        av, bv = h1[i1], a1[j][i1]
                        a1[j][i1] = cs * bv + sn * av
                        h1[i1] = cs * av - sn * bv
                        h1[i] = h1[i1]
                    h1[i1] = 0.0
                for j in range(1, kk + 1):
                    ij = n10 + j
                    if ij <= 0:
                        continue
                    piv = h2[j]
                    if piv == 0.0:
                        continue
                    cs, sn, a2[ij][j] = _givens(piv, a2[ij][j])
                    j1 = ij
                    for j2 in range(1, IDIM + 1):
                        av, bv = xi[j2], z[j1]
                        z[j1] = cs * bv + sn * av
                        xi[j2] = cs * av - sn * bv
                        j1 += n
                    if j == kk:
                        break
                    for i in range(j + 1, kk + 1):
                        av, bv = h2[i], a2[ij][i]
                        a2[ij][i] = cs * bv + sn * av
                        h2[i] = cs * av - sn * bv
                for j2 in range(1, IDIM + 1):
                    fp = fp + xi[j2] * xi[j2]
            fpint[n] = fp0
            fpint[n - 1] = fpold
            nrdata[n] = nplus
            j1 = 0
            for _ in range(IDIM):
                _back_periodic(a1, a2, z, j1, n7, kk, c, j1)
                j1 += n
            for i in range(1, k + 1):
                j1 = i
                for _ in range(IDIM):
                    c[j1 + n7] = c[j1]
                    j1 += n
            fpms = fp - s
            if abs(fpms) < acc:
                return 0, n, t, c, fp, 0.0
            if fpms < 0.0:
                part2 = True
                break
            if n == nmax:
                return -1, n, t, c, fp, 0.0
            if n == nest:
                return 1, n, t, c, fp, 0.0
            npl1 = nplus * 2
            rn = float(nplus)
            if fpold - fp > acc:
                npl1 = int(min(rn * fpms / (fpold - fp), 1073741824.0))
            nplus = min(nplus * 2, max(npl1, nplus // 2, 1))
            fpold = fp
            # residual of every knot interval, a data point on a knot shared half and half
            fpart = 0.0
            i = 1
            l = k1
            jj = 0
            new = 0
            for it in range(1, m1 + 1):
                if not u[it] < t[l]:
                    new = 1
                    l += 1
                term = 0.0
                l0 = l - k2
                for _ in range(IDIM):
                    fac = 0.0
                    j1 = l0
                    for j in range(1, k1 + 1):
                        j1 += 1
                        fac = fac + c[j1] * q[it][j]
                    jj += 1
                    d = 1.0 * (fac - x[jj])
                    term = term + d * d
                    l0 += n
                fpart = fpart + term
                if new == 0:
                    continue
                if l > k2:
                    store = term * 0.5
                    fpint[i] = fpart - store
                    i += 1
                    fpart = store
                else:
                    fpint[nrint] = term
                new = 0
            fpint[nrint] = fpint[nrint] + fpart
            for _l in range(1, nplus + 1):
                n, nrint = _new_knot(u, t, n, fpint, nrdata, nrint)
                if n == nmax:
                    restart = True
                    break
                if n == nest:
                    break
            if restart:
                break
        else:
            # m trials without an acceptable knot set: cannot happen for finite data
            return 1, n, t, c, fp, 0.0
        if restart:
            if interpolation_knots():
                return -1, n, t, c, 0.0, 0.0

    # ---- the smoothing curve: F(p) = s ------------------------------------------------------------------------------
    _disc(t, n, k2, b)
    p1, f1, p3, f3 = 0.0, fp0 - s, -1.0, fpms
    n11 = n10 - 1
    n8 = n7 - 1
    p = 0.0
    l = n7
    border_only = False
    for i in range(1, k + 1):
        j = k + 1 - i
        p = p + a2[l][j]
        l -= 1
        if l == 0:
            border_only = True
            break
    if not border_only:
        for i in range(1, n10 + 1):
            p = p + a1[i][1]
    p = float(n7) / p
    ich1 = ich3 = 0
    nc = IDIM * n
    for it_p in range(1, MAXIT + 1):
        pinv = 1.0 / p
        for i in range(1, nc + 1):
            c[i] = z[i]
        for i in range(1, n7 + 1):
            g1[i][k1] = a1[i][k1]
            g1[i][k2] = 0.0
            g2[i][1] = 0.0
            for j in range(1, k + 1):
                g1[i][j] = a1[i][j]
                g2[i][j + 1] = a2[i][j]
        l = n10
        for j in range(1, k1 + 1):
            if l <= 0:
                break
            g2[l][1] = a1[l][j]
            l -= 1
        for it in range(1, n8 + 1):
            for j in range(1, IDIM + 1):
                xi[j] = 0.0
            for i in range(1, k1 + 1):
                h1[i] = 0.0
                h2[i] = 0.0
            h1[k2] = 0.0
            if it <= n11:
                l = it
                l0 = it
                j = 1
                while j <= k2:
                    if l0 == n10:
                        l0 = 1
                        for l1 in range(j, k2 + 1):
                            h2[l0] = b[it][l1] * pinv
                            l0 += 1
                        break
                    h1[j] = b[it][j] * pinv
                    l0 += 1
                    j += 1
                rotate_band = True
            else:
                l = 1
                i = it - n10
                for j in range(1, k2 + 1):
                    i += 1
                    l0 = i
                    while True:
                        l1 = l0 - k1
                        if l1 <= 0:
                            h2[l0] = h2[l0] + b[it][j] * pinv
                            break
                        if l1 <= n11:
                            h1[l1] = b[it][j] * pinv
                            break
                        l0 = l1 - n11
                rotate_band = n11 > 0
            if rotate_band:
                for j in range(l, n11 + 1):
                    piv = h1[1]
                    cs, sn, g1[j][1] = _givens(piv, g1[j][1])
                    j1 = j
                    for j2 in range(1, IDIM + 1):
                        av, bv = xi[j2], c[j1]
                        c[j1] = cs * bv + sn * av
                        xi[j2] = cs * av - sn * bv
                        j1 += n
                    for i in range(1, k1 + 1):
                        av, bv = h2[i], g2[j][i]
                        g2[j][i] = cs * bv + sn * av
                        h2[i] = cs * av - sn * bv
                    if j == n11:
                        break
                    i2 = min(n11 - j, k1)
                    i1 = 1
                    for i in range(1, i2 + 1):
                        i1 = i + 1
                        av, bv = h1[i1], g1[j][i1]
                        g1[j][i1] = cs * bv + sn * av
                        h1[i1] = cs * av - sn * bv
                        h1[i] = h1[i1]
                    h1[i1] = 0.0
            for j in range(1, k1 + 1):
                ij = n11 + j
                if ij <= 0:
                    continue
                piv = h2[j]
                cs, sn, g2[ij][j] = _givens(piv, g2[ij][j])
                j1 = ij
                for j2 in range(1, IDIM + 1):
                    av, bv = xi[j2], c[j1]
                    c[j1] = cs * bv + sn * av
                    xi[j2] = cs * av - sn * bv
                    j1 += n
                if j == k1:
                    break
                for i in range(j + 1, k1 + 1):
                    av, bv = h2[i], g2[ij][i]
                    g2[ij][i] = cs * bv + sn * av
                    h2[i] = cs * av - sn * bv
        j1 = 0
        for _ in range(IDIM):
            _back_periodic(g1, g2, c, j1, n7, k1, c, j1)
            j1 += n
        for i in range(1, k + 1):
            j1 = i
            for _ in range(IDIM):
                c[j1 + n7] = c[j1]
                j1 += n
        fp = 0.0
        l = k1
        jj = 0
        for it in range(1, m1 + 1):
            if not u[it] < t[l]:
                l += 1
            l0 = l - k2
            term = 0.0
            for _ in range(IDIM):
                fac = 0.0
                j1 = l0
                for j in range(1, k1 + 1):
                    j1 += 1
                    fac = fac + c[j1] * q[it][j]
                jj += 1
                d = fac - x[jj]
                term = term + d * d
                l0 += n
            fp = fp + term * (1.0 * 1.0)
        fpms = fp - s
        if abs(fpms) < acc:
            return 0, n, t, c, fp, p
        if it_p == MAXIT:
            return 3, n, t, c, fp, p
        p2, f2 = p, fpms
        if ich3 == 0:
            if not (f2 - f3) > acc:
                p3, f3 = p2, f2
                p = p * 0.04
                if p <= p1:
                    p = p1 * 0.9 + p2 * 0.1
                continue
            if f2 < 0.0:
                ich3 = 1
        if ich1 == 0:
            if not (f1 - f2) > acc:
                p1, f1 = p2, f2
                p = p / 0.04
                if p3 < 0.0:
                    continue
                if p >= p3:
                    p = p2 * 0.1 + p3 * 0.9
                continue
            if f2 > 0.0:
                ich1 = 1
        if f2 >= f1 or f2 <= f3:
            return 2, n, t, c, fp, p
        p, p1, f1, p3, f3 = _rati(p1, f1, p2, f2, p3, f3)
    return 3, n, t, c, fp, p


def _evaluate(t, n, c, k, m):
    """the curve at i * (1 / m), i = 0..m-1 (numpy's linspace(0, 1, m, endpoint=False))"""
    k1 = k + 1
    nk1 = n - k1
    out = np.empty((m, 3))
    h = [0.0] * (k + 3)
    hh = [0.0] * (k + 3)
    step = 1.0 / float(m)
    l = k1
    for i in range(m):
        arg = float(i) * step
        while not (arg < t[l + 1] or l == nk1):
            l += 1
        _bspl(t, k, arg, l, h, hh)
        for d in range(IDIM):
            sp = 0.0
            ll = l - k1 + d * n
            for j in range(1, k1 + 1):
                ll += 1
                sp = sp + c[ll] * h[j]
            out[i, d] = sp
    return out


def fit_closed(points, smoothing: float = 0.0, degree: int = 3) -> dict:
    """One contour -> {"status", "points", "centroid", "fp", "n_knots", "knots", "coef" (1-based, three blocks of
    n_knots), "ier", "p"}.  An unchanged contour
    comes back as a copy of its input with fp = 0, no knots and the centroid of its own points."""
    k = int(degree)
    s = float(smoothing)
    if not 1 <= k <= 5:
        raise ValueError("degree must be in 1..5")
    if not (s >= 0.0) or math.isinf(s):
        raise ValueError("smoothing must be finite and >= 0")
    pts = np.ascontiguousarray(np.asarray(points, dtype=np.float64).reshape(-1, 3))
    m = pts.shape[0]
    if m > MAX_POINTS:
        raise ValueError("more than MAX_POINTS points")

    def unchanged(status):
        cen = tuple(pairwise_mean(pts[:, d]) for d in range(3)) if m else (float("nan"),) * 3
        return {"status": status, "points": pts.copy(), "centroid": cen, "fp": 0.0, "n_knots": 0,
                "knots": np.zeros(0), "coef": [], "ier": None, "p": 0.0}

    if m < k + 1:
        return unchanged(UNCHANGED_SHORT)
    if not np.isfinite(pts).all():
        return unchanged(UNCHANGED_NONFINITE)
    x = [0.0] * (IDIM * m + 1)
    for i in range(m):
        src = 0 if i == m - 1 else i                       # the last point gives way to the first
        for d in range(IDIM):
            x[IDIM * i + d + 1] = float(pts[src, d])
    u = [0.0] * (m + 1)
    for i in range(2, m + 1):
        dist = 0.0
        for d in range(1, IDIM + 1):
            dd = x[IDIM * (i - 1) + d] - x[IDIM * (i - 2) + d]
            dist = dist + dd * dd
        u[i] = u[i - 1] + math.sqrt(dist)
    if not u[m] > 0.0:
        return unchanged(UNCHANGED_ZERO_CHORD)
    total = u[m]
    if not math.isfinite(total):                           # finite coordinates whose squared chord overflows
        return unchanged(UNCHANGED_NONFINITE)
    for i in range(2, m + 1):
        u[i] = u[i] / total
    u[m] = 1.0
    for i in range(2, m + 1):
        if not math.isfinite(u[i]):
            return unchanged(UNCHANGED_NONFINITE)
        if u[i - 1] >= u[i]:
            return unchanged(UNCHANGED_ZERO_CHORD)
    try:
        ier, n, t, c, fp, p = _closed_curve(x, u, m, k, s)
        out = _evaluate(t, n, c, k, m)
    except ZeroDivisionError:                       # a singular system (scipy returns NaN coefficients there)
        return unchanged(UNCHANGED_NONFINITE)
    if not (np.isfinite(out).all() and math.isfinite(fp)):
        return unchanged(UNCHANGED_NONFINITE)
    cen = tuple(pairwise_mean(out[:, d]) for d in range(3))
    return {"status": status_of_ier(ier), "points": out, "centroid": cen, "fp": fp, "n_knots": n,
            "knots": np.array(t[1:n + 1]), "coef": c, "ier": ier, "p": p}


def fit_closed_batch(contours, smoothing: float = 0.0, degree: int = 3) -> list:
    return [fit_closed(c, smoothing, degree) for c in contours]
