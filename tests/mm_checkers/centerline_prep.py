"""Plain-Python restatement of the centerline's branch structure (src/types/native/centerline.rs:64-937), of
prepare_centerline (multimodars/ccta/centerline_prep.py:54-134) and of the branch masks and lists of label_branches
(multimodars/ccta/labeling.py:415-487, src/ccta/adjust_mesh/label_coronary.rs:201-235): the yardstick for
csrc/mm_cl_branches.cpp, csrc/mm_branch_kernels.hip and csrc/mm_branch.cpp.  Written from the reference, with its own data
layout: a centerline is a `CL` holding points (x, y, z, radius), their branch ids, tangents and, as in the reference, an
explicit list of branch start indices.  Every float operation is a Python float operation in the reference's order:
distances are sqrt((dx dx + dy dy) + dz dz), sums run in index order, minima are first minima (strict <).
"""
import math
from collections import deque

import numpy as np


class CL:
    def __init__(self, pts, branch_id, starts, tangents=None):
        self.pts = [tuple(float(v) for v in p) for p in pts]              # (x, y, z, radius)
        self.branch_id = [int(b) for b in branch_id]
        self.starts = list(starts)
        self.tangents = [tuple(t) for t in tangents] if tangents is not None else [(0.0, 0.0, 0.0)] * len(self.pts)

    @staticmethod
    def from_branches(branches):
        """make_multi_branch of the reference's tests: branches of (x, y, z) or (x, y, z, radius), zero tangents."""
        pts, bid, starts = [], [], []
        for b, br in enumerate(branches):
            starts.append(len(pts))
            for p in br:
                pts.append(tuple(p) + (0.0,) * (4 - len(p)))
                bid.append(b)
        return CL(pts, bid, starts)

    @staticmethod
    def from_coords(coords):
        """Centerline::from_contour_points (:14-42)"""
        pts = [tuple(p) + (0.0,) for p in coords]
        tan = []
        for i in range(len(pts)):
            if i + 1 < len(pts):
                tan.append(_unit(_sub(pts[i + 1], pts[i])))
            else:
                tan.append(tan[i - 1])
        return CL(pts, [0] * len(pts), [0] if pts else [], tan)

    def branches(self):
        ends = self.starts[1:] + [len(self.pts)]
        return [list(self.pts[s:e]) for s, e in zip(self.starts, ends)]

    def copy(self):
        return CL(self.pts, self.branch_id, self.starts, self.tangents)


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _norm(v):
    return math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def _unit(v):
    n = _norm(v)
    return tuple(_div(c, n) for c in v)


def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:                                             # IEEE: x / 0 = inf, 0 / 0 = nan
        return math.nan if a == 0.0 or a != a else math.copysign(math.inf, a) * math.copysign(1.0, b)


def dist(a, b):
    return _norm(_sub(a, b))


def recompute_tangents(cl):
    n = len(cl.pts)
    for i in range(n):
        if i + 1 < n and cl.branch_id[i] == cl.branch_id[i + 1]:
            cl.tangents[i] = _unit(_sub(cl.pts[i + 1], cl.pts[i]))
        elif i > 0 and cl.branch_id[i - 1] == cl.branch_id[i]:
            cl.tangents[i] = cl.tangents[i - 1]
        else:
            cl.tangents[i] = (0.0, 0.0, 0.0)


def rebuild(branches):
    pts, bid, starts = [], [], []
    for b, br in enumerate(branches):
        starts.append(len(pts))
        pts += br
        bid += [b] * len(br)
    cl = CL(pts, bid, starts)
    recompute_tangents(cl)
    return cl


# ---- calculate_branches (:78-339) ----------------------------------------------------------------------------------------

def p95_spacing(pts):
    if len(pts) < 2:
        return 1.0
    s = sorted(dist(pts[i - 1], pts[i]) for i in range(1, len(pts)))
    return s[len(s) * 95 // 100]


def _bfs_farthest(pts, adj, start):
    d = [math.inf] * len(pts)
    prev = [None] * len(pts)
    d[start] = 0.0
    q = deque([start])
    far = start
    while q:
        u = q.popleft()
        for v in adj[u]:
            if math.isinf(d[v]):
                d[v] = d[u] + dist(pts[u], pts[v])
                prev[v] = u
                q.append(v)
                if d[v] > d[far]:
                    far = v
    return far, prev


def _order_chain(comp, adj):
    inside = set(comp)
    start = next((i for i in comp if sum(1 for nb in adj[i] if nb in inside) <= 1), comp[0])
    ordered, seen, cur = [], set(), start
    while True:
        ordered.append(cur)
        seen.add(cur)
        nxt = next((nb for nb in adj[cur] if nb in inside and nb not in seen), None)
        if nxt is None:
            break
        cur = nxt
    return ordered + [i for i in comp if i not in seen]


def calculate_branches(cl, spacing_tolerance):
    pts, n = cl.pts, len(cl.pts)
    if n == 0:
        return CL([], [], [])
    threshold = p95_spacing(pts) * spacing_tolerance
    seg = [0] + [i for i in range(1, n) if dist(pts[i - 1], pts[i]) > threshold] + [n]
    adj = [[] for _ in range(n)]
    for i in range(1, n):
        if dist(pts[i - 1], pts[i]) <= threshold:
            adj[i - 1].append(i)
            adj[i].append(i - 1)
    for si in range(len(seg) - 1):
        for sj in range(si + 1, len(seg) - 1):
            best, bi, bj = math.inf, seg[si], seg[sj]
            for pi in range(seg[si], seg[si + 1]):
                for pj in range(seg[sj], seg[sj + 1]):
                    d = dist(pts[pi], pts[pj])
                    if d < best:
                        best, bi, bj = d, pi, pj
            if best <= threshold:
                adj[bi].append(bj)
                adj[bj].append(bi)
    a, _ = _bfs_farthest(pts, adj, 0)
    b, prev = _bfs_farthest(pts, adj, a)
    main, cur = [], b
    while True:
        main.append(cur)
        if cur == a or prev[cur] is None:
            break
        cur = prev[cur]
    visited = [False] * n
    for i in main:
        visited[i] = True
    comps = []
    for s in range(n):
        if visited[s]:
            continue
        comp, q = [], deque([s])
        visited[s] = True
        while q:
            u = q.popleft()
            comp.append(u)
            for v in adj[u]:
                if not visited[v]:
                    visited[v] = True
                    q.append(v)
        comps.append(comp)
    real = sorted((c for c in comps if len(c) >= 5), key=lambda c: -len(c))          # stable
    return rebuild([[pts[i] for i in main]] + [[pts[i] for i in _order_chain(c, adj)] for c in real])


# ---- the editing methods ---------------------------------------------------------------------------------------------------

def find_sharp_angles(cl, branch_id, cos_threshold):
    if branch_id >= len(cl.starts):
        return []
    start = cl.starts[branch_id]
    end = cl.starts[branch_id + 1] if branch_id + 1 < len(cl.starts) else len(cl.pts)
    out = []
    for i in range(start + 1, end - 1):
        v1, v2 = _sub(cl.pts[i - 1], cl.pts[i]), _sub(cl.pts[i + 1], cl.pts[i])
        n1, n2 = _norm(v1), _norm(v2)
        if n1 < 1e-10 or n2 < 1e-10:
            continue
        if (v1[0] * v2[0] + v1[1] * v2[1] + v1[2] * v2[2]) / (n1 * n2) > cos_threshold:
            out.append(i)
    return out


def split_branch(cl, branch_id, point_index):
    br = cl.branches()
    if branch_id >= len(br):
        return cl.copy()
    start = cl.starts[branch_id]
    if point_index < start or point_index >= start + len(br[branch_id]):
        return cl.copy()
    local = point_index - start
    whole = br.pop(branch_id)
    if local == 0 or local >= max(len(whole) - 1, 0):
        return cl.copy()
    br += [whole[:local + 1], whole[local:]]
    br.sort(key=lambda b: -len(b))
    return rebuild(br)


def merge_branches(cl, a, b):
    br = cl.branches()
    if a == b or a >= len(br) or b >= len(br):
        return cl.copy()
    lo, hi = min(a, b), max(a, b)
    bh = br.pop(hi)
    bl = br.pop(lo)
    d = [dist(bl[-1], bh[0]), dist(bl[-1], bh[-1]), dist(bl[0], bh[0]), dist(bl[0], bh[-1])]
    m = d[0]
    for x in d[1:]:
        m = x if x < m or m != m else m                                    # f64::min ignores a NaN
    if abs(m - d[0]) < 1e-12:
        merged = bl + bh
    elif abs(m - d[1]) < 1e-12:
        merged = bl + bh[::-1]
    elif abs(m - d[2]) < 1e-12:
        merged = bh[::-1] + bl
    else:
        merged = bh + bl
    br.append(merged)
    br.sort(key=lambda x: -len(x))
    return rebuild(br)


def _reverse_by_max_z(b):
    best = 0
    for i in range(1, len(b)):
        if not b[best][2] > b[i][2]:                                       # max_by keeps the last maximum
            best = i
    return best != 0


def _reverse_relative_to(b, ref):
    if not b or not ref:
        return False
    df = dl = math.inf
    for p in ref:
        x = dist(p, b[0])
        df = x if x < df else df
    for p in ref:
        x = dist(p, b[-1])
        dl = x if x < dl else dl
    return dl < df


def orient_by_max_z(cl):
    br = cl.branches()
    if not br:
        return cl.copy()
    if _reverse_by_max_z(br[0]):
        br[0].reverse()
    for b in br[1:]:
        if _reverse_relative_to(b, br[0]):
            b.reverse()
    return rebuild(br)


def orient_to_reference(cl, reference):
    br = cl.branches()
    if not br:
        return cl.copy()
    end = reference.starts[1] if len(reference.starts) > 1 else len(reference.pts)
    ref0 = reference.pts[:end]
    for b in br:
        if _reverse_relative_to(b, ref0):
            b.reverse()
    return rebuild(br)


def mean_spacing(cl):
    end = cl.starts[1] if len(cl.starts) > 1 else len(cl.pts)
    if end < 2:
        return 1.0
    s = 0.0
    for i in range(1, end):
        s += dist(cl.pts[i - 1], cl.pts[i])
    return s / (end - 1)


def remove_branch_overlap(cl):
    if not cl.starts:
        return cl.copy()
    buf = mean_spacing(cl)
    buf2 = buf * buf
    br = cl.branches()
    if len(br) > 1:
        known = list(br[0])
        for k in range(1, len(br)):
            def close(p):
                return any((p[0] - m[0]) * (p[0] - m[0]) + (p[1] - m[1]) * (p[1] - m[1]) + (p[2] - m[2]) * (p[2] - m[2]) <= buf2
                           for m in known)
            j = next((i for i, p in enumerate(br[k]) if not close(p)), None)
            if j is None:
                br[k] = []
            elif j > 0:
                br[k] = br[k][j - 1:]
            known += br[k]
        br = [b for b in br if b]
    return rebuild(br)


def trim_start(cl, mm):
    if mm <= 0.0 or not cl.starts:
        return cl.copy()
    br = cl.branches()
    if len(br[0]) > 1:
        arc, trim = 0.0, 0
        for i in range(1, len(br[0])):
            arc += dist(br[0][i - 1], br[0][i])
            if arc <= mm:
                trim = i
            else:
                break
        br[0] = br[0][trim:]
    return rebuild(br)


def resample(cl, spacing_mm):
    """Centerline::resample (:717-790)"""
    if not cl.pts or spacing_mm <= 1e-12:
        return cl.copy()
    out = []
    for pts in cl.branches():
        if len(pts) < 2:
            out.append(pts)
            continue
        cum = [0.0]
        for i in range(1, len(pts)):
            cum.append(cum[-1] + dist(pts[i - 1], pts[i]))
        total = cum[-1]
        if total < 1e-12:
            out.append(pts)
            continue
        targets, s = [], 0.0
        while s < total:
            targets.append(s)
            s += spacing_mm
        targets.append(total)
        seg, res = 0, []
        for t in targets:
            while seg < len(pts) - 2 and cum[seg + 1] < t:
                seg += 1
            s0, s1 = cum[seg], cum[seg + 1]
            f = 0.0 if abs(s1 - s0) < 1e-12 else (t - s0) / (s1 - s0)
            p0, p1 = pts[seg], pts[seg + 1]
            res.append(tuple(p0[c] + f * (p1[c] - p0[c]) for c in range(4)))
        out.append(res)
    return rebuild(out)


def smooth(cl, sigma):
    if not cl.pts or sigma < 1e-12:
        return cl.copy()
    out = cl.copy()
    new = list(cl.pts)
    r3 = math.ceil(3.0 * sigma) if sigma == sigma and not math.isinf(sigma) else (0 if sigma != sigma else 1 << 62)
    for b in range(max(cl.branch_id) + 1):
        idx = [i for i, x in enumerate(cl.branch_id) if x == b]
        for li, gi in enumerate(idx):
            r = min(li, r3, len(idx) - 1 - li)
            wx = wy = wz = wt = 0.0
            for j in range(li - r, li + r + 1):
                diff = float(li) - float(j)
                w = math.exp(-0.5 * diff * diff / (sigma * sigma))
                p = cl.pts[idx[j]]
                wx += w * p[0]
                wy += w * p[1]
                wz += w * p[2]
                wt += w
            if wt > 1e-12:
                new[gi] = (wx / wt, wy / wt, wz / wt, cl.pts[gi][3])
    out.pts = new
    recompute_tangents(out)
    return out


def prepare_centerline(cl, ref=None, spacing_mm=None, branch_spacing_tolerance=2.0, rm_start_mm=0.0, smooth_sigma=2.5,
                       trace=None):
    """centerline_prep.py:113-134; `trace` (a list) receives the names of the steps that ran."""
    def step(name, fn, *a):
        if trace is not None:
            trace.append(name)
        return fn(*a)
    if ref is not None and len(cl.starts) <= 1:
        cl = step("calculate_branches", calculate_branches, cl, branch_spacing_tolerance)
    cl = step("remove_branch_overlap", remove_branch_overlap, cl)
    if rm_start_mm > 0:
        cl = step("trim_start", trim_start, cl, rm_start_mm)
    if spacing_mm:
        cl = step("resample", resample, cl, spacing_mm)
    if ref is not None:
        cl = step("orient_to_reference", orient_to_reference, cl, ref)
    else:
        cl = step("orient_by_max_z", orient_by_max_z, cl)
    if smooth_sigma > 0:
        cl = step("smooth", smooth, cl, smooth_sigma)
    return cl


# ---- branch masks and the lists of label_branches --------------------------------------------------------------------------

def branch_masks(cl_xyz, cl_branch, pts, radius):
    """bit b of mask[i]: some centerline point of branch b has dx dx + dy dy + dz dz <= radius radius, d = point -
    centerline point (label_coronary.rs:218-228), one numpy f64 operation per reference operation."""
    c = np.asarray(cl_xyz, dtype=np.float64).reshape(-1, 3)
    b = np.asarray(cl_branch, dtype=np.int64).reshape(-1)
    p = np.asarray(pts, dtype=np.float64).reshape(-1, 3)
    if b.size and (b.max() >= 64 or b.min() < 0):
        raise ValueError("a mask holds 64 branches")
    r2 = np.float64(radius) * np.float64(radius)
    mask = np.zeros(p.shape[0], dtype=np.uint64)
    with np.errstate(over="ignore", invalid="ignore"):
        for j in range(c.shape[0]):
            dx, dy, dz = p[:, 0] - c[j, 0], p[:, 1] - c[j, 1], p[:, 2] - c[j, 2]
            v = dx * dx + dy * dy + dz * dz
            mask[v <= r2] |= np.uint64(1) << np.uint64(b[j])
    return mask


def select(masks, main_ids, n_branches):
    """(main, side, {k: side_k}) index arrays of labeling.py:465-484 from the masks"""
    masks = np.asarray(masks, dtype=np.uint64)
    main_bits = np.uint64(0)
    for b in main_ids:
        main_bits |= np.uint64(1) << np.uint64(b)
    is_main = (masks & main_bits) != 0
    side = np.flatnonzero(~is_main)
    side_k = {k: side[(masks[side] >> np.uint64(k)) & np.uint64(1) == 1]
              for k in range(n_branches) if k not in set(main_ids)}
    return np.flatnonzero(is_main), side, side_k
