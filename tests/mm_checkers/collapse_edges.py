"""Plain Python restatement of the mesh edge collapse (include/mm_ccta.h, "mesh edge collapse"): the yardstick for
csrc/mm_collapse_kernels.hip and csrc/mm_collapse.cpp.  Every f64 operation is an operation on Python floats: IEEE
doubles, unfused, one rounding each, in the header's order -- the cross product, dot, len_sq and the quality of
flip_edges.py and refine_mesh.py restated on floats, which a pass over dozens of passes needs for its speed (a test
holds the two forms against each other).  The edge table and the valences are those of flip_edges.py.

* `neighbourhoods`: per vertex its ring, its faces, whether it is removable.
* `direction`: the guards (c) .. (g) of one direction r -> k, stated as "for all" over the ring: 0 or the class that failed.
* `one_pass`: the short edges, the candidates with their direction and priority, the blocked counts, what collapses.
* `collapse`: the passes, the compaction, origin, target and the report; with `trace=True` also what every pass found.
* `predict_report`: the fields the data does not decide (launches, bytes).
"""
import struct

import numpy as np

from . import flip_edges as FE
from . import smooth_mesh as SMO

PASS_LAUNCHES = 10              # edge table, valences, the adjacency (6), candidates, collapses
STAT_LAUNCHES = 2               # edge table, valences: the state behind the last of max_passes
END_LAUNCHES = 9                # two scans (3 each), the gather, the remap, origin and target
SLOTS = 16
COUNTER_BYTES = 128
BLOCKS = ("blocked_fixed", "blocked_link", "blocked_valence", "blocked_long", "blocked_normal", "blocked_quality")
EDGE_KEYS = ("n_edges", "n_open_edges", "n_nonmanifold_edges", "n_inconsistent_edges")
MIN_RATIO, MAX_RATIO = 4.0 / 5.0, 4.0 / 3.0
crease_cos = FE.crease_cos
INF = float("inf")


def sub(p, q):
    return (p[0] - q[0], p[1] - q[1], p[2] - q[2])


def cross(u, w):
    return (u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0])


def dot(u, w):
    return (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2]


def len_sq(p, q):
    """((dx dx + dy dy) + dz dz) of d = q - p."""
    dx, dy, dz = q[0] - p[0], q[1] - p[1], q[2] - p[2]
    return (dx * dx + dy * dy) + dz * dz


def quality(v, i, j, k, n):
    """dot(n, n) / (S S), S = (len_sq(i, j) + len_sq(j, k)) + len_sq(k, i); 0 where S is 0.  S S may be 0 or infinite
    where S is neither: the division is IEEE's."""
    s = (len_sq(v[i], v[j]) + len_sq(v[j], v[k])) + len_sq(v[k], v[i])
    if s == 0.0:
        return 0.0
    with np.errstate(all="ignore"):
        return dot(n, n) / (s * s) if s * s != 0.0 else float(np.float64(dot(n, n)) / np.float64(s * s))


def thresholds(target_len, min_ratio=MIN_RATIO, max_ratio=MAX_RATIO):
    """(thr_min2, thr_max2), each computed once."""
    a, b = float(min_ratio) * float(target_len), float(max_ratio) * float(target_len)
    return a * a, b * b


def bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def neighbourhoods(f, nv, table, mask):
    """(nbr: a set per vertex, at: the faces with a corner at the vertex, deg, border, removable)."""
    deg, border, _ = FE.valence([], nv, table, None)
    nbr = [set() for _ in range(nv)]
    twisted = np.zeros(nv, dtype=bool)
    for (lo, hi), e in table.items():
        if lo != hi:
            nbr[lo].add(hi)
            nbr[hi].add(lo)
        if e["n"] == 2 and e["own"][0][1] == e["own"][1][1]:              # an (a, a) edge owned twice: both bits are 0
            twisted[lo] = twisted[hi] = True
    at = [[] for _ in range(nv)]
    for i, face in enumerate(f):
        for x in set(face):
            at[x].append(i)
    removable = [not (mask is not None and mask[x]) and not border[x] and not twisted[x] and deg[x] >= 3 for x in range(nv)]
    return nbr, at, deg.tolist(), border.tolist(), removable


def direction(v, f, r, k, c, d, owners, nbr, at, deg, border, table, thr_max2, cc2, qk2):
    """(0 or 1 .. 5 for the first of (c) .. (g) that fails, the longest new squared length) of the collapse r -> k."""
    if nbr[r] & nbr[k] != {c, d}:                                                              # (c)
        return 1, 0.0
    if not (deg[k] + deg[r] - 4 >= 3 and deg[c] - 1 >= (2 if border[c] else 3) and deg[d] - 1 >= (2 if border[d] else 3)):
        return 2, 0.0                                                                       # (d)
    longest, fail = 0.0, 0
    for n in nbr[r] - {k, c, d}:                                                               # (e)
        x = len_sq(v[k], v[n])
        if not x <= thr_max2:
            fail = 3
        elif x > longest:
            longest = x
    if fail:
        return fail, longest
    q_new, t_old, nan = INF, INF, False
    for i in at[r]:
        face = f[i]
        j = face.index(r)
        x, y = face[(j + 1) % 3], face[(j + 2) % 3]
        n_old = cross(sub(v[x], v[r]), sub(v[y], v[r]))
        t = qk2 * quality(v, r, x, y, n_old)
        nan = nan or t != t
        t_old = t if t < t_old else t_old
        if i in owners:
            continue
        n_new = cross(sub(v[x], v[k]), sub(v[y], v[k]))
        dn = dot(n_old, n_new)
        if not (dn > 0.0 and dn * dn >= cc2 * (dot(n_old, n_old) * dot(n_new, n_new))):       # (f)
            fail = 4
        qn = quality(v, k, x, y, n_new)
        nan = nan or qn != qn
        q_new = qn if qn < q_new else q_new
    if fail:
        return fail, longest
    return (5 if nan or not q_new >= t_old else 0), longest                                    # (g): the two minima


def one_pass(v, f, alive, mask, thr_min2, thr_max2, cc2, qk2):
    """One pass over the faces f (a list of triples; alive: which of them still exist) as they are: {"short": [...],
    "candidates": [...], "collapsed": [...], the blocked counts, "reason": {blocked edge: which count}, "info": the edge
    counts}.  A candidate is a dict of lo, hi, r, k, c, d, fp, fm, ring, faces (those at r), prio."""
    nv = len(v)
    table = FE.edge_table([t for t, a in zip(f, alive) if a])
    ids = [i for i, a in enumerate(alive) if a]
    for e in table.values():                                              # faces killed before are not inserted: the ids
        e["first"] = 3 * ids[e["first"] // 3] + e["first"] % 3            # of the survivors are those of the input
        e["own"] = [(ids[i], way) for i, way in e["own"]]
    info = {k: x for k, x in FE.valence([t for t, a in zip(f, alive) if a], nv, None, None)[2].items() if k in EDGE_KEYS}
    nbr, at, deg, border, removable = neighbourhoods([t if a else () for t, a in zip(f, alive)], nv, table, mask)
    out = {"short": [], "candidates": [], "reason": {}, "info": info, **{k: 0 for k in BLOCKS}}

    def block(edge, why):
        out[why] += 1
        out["reason"][edge] = why

    for (lo, hi), e in table.items():
        if lo == hi or not len_sq(v[lo], v[hi]) < thr_min2:
            continue
        out["short"].append((lo, hi))
        if not (removable[lo] or removable[hi]):
            block((lo, hi), "blocked_fixed")
            continue
        ok = e["n"] == 2 and e["own"][0][1] != e["own"][1][1]                             # (a)
        if ok:
            fp, fm = (e["own"][0][0], e["own"][1][0]) if e["own"][0][1] else (e["own"][1][0], e["own"][0][0])
            ok = len(set(f[fp])) == 3 and len(set(f[fm])) == 3
        if ok:
            c, d = sum(f[fp]) - lo - hi, sum(f[fm]) - lo - hi
            ok = c != d
        if not ok:                                                    # no link of two vertices: counted with (c)
            block((lo, hi), "blocked_link")
            continue
        res = {}
        for r, k in ((hi, lo), (lo, hi)):
            if removable[r]:                                          # (b)
                res[r] = direction(v, f, r, k, c, d, (fp, fm), nbr, at, deg, border, table, thr_max2, cc2, qk2)
        good = [r for r in (hi, lo) if r in res and res[r][0] == 0]
        if not good:
            block((lo, hi), BLOCKS[res[hi][0] if hi in res else res[lo][0]])
            continue
        r = good[0] if len(good) == 1 or not res[lo][1] < res[hi][1] else lo              # ties: r = hi
        prio = ((0xFFFFFFFF - (bits(len_sq(v[lo], v[hi])) >> 32)) << 32) | (0xFFFFFFFF - e["first"])
        out["candidates"].append(dict(lo=lo, hi=hi, r=r, k=lo + hi - r, c=c, d=d, fp=fp, fm=fm, ring=sorted(nbr[r]),
                                      faces=list(at[r]), prio=prio))
    best = {}
    for k in out["candidates"]:
        for x in [k["r"]] + k["ring"]:
            best[x] = max(best.get(x, 0), k["prio"])
    out["collapsed"] = [k for k in out["candidates"] if all(best[x] == k["prio"] for x in [k["r"]] + k["ring"])]
    return out


def rewrite(f, alive, collapsed):
    """The faces and their liveness after the collapses: r <- k in every face at r, the two owners die."""
    f, alive = list(f), list(alive)
    for k in collapsed:
        for i in k["faces"]:
            f[i] = tuple(k["k"] if x == k["r"] else x for x in f[i])
        alive[k["fp"]] = alive[k["fm"]] = False
    return f, alive


def predict_report(nv, nf, nv_out, nf_out, passes_run, converged, masked=False):
    """n_launches, bytes_uploaded and bytes_downloaded as the header states them."""
    if nv == 0 or nf == 0:
        return dict(n_launches=0, bytes_uploaded=0, bytes_downloaded=0)
    return dict(n_launches=PASS_LAUNCHES * passes_run + (0 if converged else STAT_LAUNCHES) + END_LAUNCHES +
                SMO.volume_launches(nf) + (SMO.volume_launches(nf_out) if nf_out else 0),
                bytes_uploaded=24 * nv + 12 * nf + (nv if masked else 0),
                bytes_downloaded=28 * nv_out + 12 * nf_out + 4 * nv + COUNTER_BYTES)


def collapse(v, f, target_len, mask=None, min_ratio=MIN_RATIO, max_ratio=MAX_RATIO, crease_cos=crease_cos(), quality_keep=0.5,
             max_passes=50, trace=False):
    """(vertices (kv, 3), faces (kf, 3) int64, origin (kv,), target (nv,), report[, one one_pass result per pass run])."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    nv, nf = v.shape[0], f.shape[0]
    pv = [tuple(p) for p in v.tolist()]                                  # the coordinates as Python floats
    mask = None if mask is None else (np.asarray(mask).reshape(-1) != 0).tolist()
    thr_min2, thr_max2 = thresholds(target_len, min_ratio, max_ratio)
    cc2, qk2 = float(crease_cos) * float(crease_cos), float(quality_keep) * float(quality_keep)
    rep = {"n_vertices": nv, "n_faces": nf, "passes_run": 0, "converged": 0, "n_collapses": 0,
           "collapses_per_pass": [0] * SLOTS, "candidates_per_pass": [0] * SLOTS, **{k: 0 for k in BLOCKS}}
    cf = [tuple(int(x) for x in t) for t in f.tolist()]
    alive, to = [True] * nf, list(range(nv))
    device = nv > 0 and nf > 0
    passes, first, last = [], None, None
    while device and rep["passes_run"] < int(max_passes):
        p = one_pass(pv, cf, alive, mask, thr_min2, thr_max2, cc2, qk2)
        passes.append(p)
        first = first or dict(p["info"], n_short=len(p["short"]))
        slot = min(rep["passes_run"], SLOTS - 1)
        rep["passes_run"] += 1
        rep["candidates_per_pass"][slot] += len(p["candidates"])
        rep["collapses_per_pass"][slot] += len(p["collapsed"])
        rep["n_collapses"] += len(p["collapsed"])
        for k in BLOCKS:
            rep[k] += p[k]
        if not p["candidates"]:
            rep["converged"] = 1
            last = len(p["short"])
            break
        cf, alive = rewrite(cf, alive, p["collapsed"])
        for k in p["collapsed"]:
            to[k["r"]] = k["k"]
    if device and not rep["converged"]:
        live = [t for t, a in zip(cf, alive) if a]
        with np.errstate(all="ignore"):
            last = sum(1 for (lo, hi) in FE.edge_table(live) if lo != hi and len_sq(pv[lo], pv[hi]) < thr_min2)
        first = first or dict({k: x for k, x in FE.valence(live, nv)[2].items() if k in EDGE_KEYS}, n_short=last)
    first = first or dict({k: 0 for k in EDGE_KEYS}, n_short=0)
    keep = np.ones(nv, dtype=bool)
    root = np.arange(nv, dtype=np.int64)
    for x in range(nv):
        t = x
        while to[t] != t:                                                 # chains across the passes
            t = to[t]
        root[x] = t
        keep[x] = t == x
    origin = np.flatnonzero(keep).astype(np.int64)
    index = np.cumsum(keep) - 1
    target = index[root].astype(np.int64)
    out_v = v[origin].copy()
    live = np.array([t for t, a in zip(cf, alive) if a], dtype=np.int64).reshape(-1, 3)
    out_f = index[live].astype(np.int64).reshape(-1, 3)
    for k in EDGE_KEYS:
        rep[k] = first[k]
    rep.update(n_vertices_out=len(origin), n_faces_out=len(out_f), n_short_before=first["n_short"], n_short_after=last or 0,
               volume_before=SMO.volume(v, f) if device else 0.0,
               volume_after=SMO.volume(out_v, out_f) if device and len(out_f) else 0.0,
               **predict_report(nv, nf, len(origin), len(out_f), rep["passes_run"], rep["converged"], mask is not None))
    res = (out_v, out_f, origin, target, rep)
    return res + (passes,) if trace else res
