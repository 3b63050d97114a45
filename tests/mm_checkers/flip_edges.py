"""Plain Python / numpy restatement of the mesh edge flips (include/mm_ccta.h, "mesh edge flips"): the yardstick for
csrc/mm_flip_kernels.hip and csrc/mm_flip.cpp.  Every f64 operation is a numpy scalar operation: IEEE, unfused, one
rounding a line, in the header's order.

* `edge_table`: per undirected edge its owners (face, direction), its owner count and `first`, the smallest corner id.
* `valence`: deg, border, ex and the deviation; the edge counts of the report.
* `one_pass`: the candidates with their gain and priority, what each guard blocked, the edges that flip.
* `flip`: the passes and the report; with `trace=True` also what every pass found.
* `predict_report`: the fields the data does not decide (launches, bytes).
"""
import math

import numpy as np

from . import smooth_mesh as SMO
from .refine_mesh import len_sq

PASS_LAUNCHES = 5               # edge table, valences, deviation, candidates, flips
STAT_LAUNCHES = 3               # edge table, valences, deviation: mesh_valence, and the state behind the last of max_passes
SLOTS = 16
COUNTER_BYTES = 128
GAIN_CAP = 1 << 20
BLOCKS = ("blocked_existing", "blocked_normal", "blocked_crease", "blocked_quality")
F = np.float64


def crease_cos(crease_deg=30.0):
    return math.cos(math.radians(float(crease_deg)))


def sub(p, q):
    return (F(p[0]) - F(q[0]), F(p[1]) - F(q[1]), F(p[2]) - F(q[2]))


def cross(u, w):
    return (u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0])


def dot(u, w):
    return (u[0] * w[0] + u[1] * w[1]) + u[2] * w[2]


def quality(v, i, j, k, n):
    """dot(n, n) / (S S), S = (len_sq(i, j) + len_sq(j, k)) + len_sq(k, i); 0 where S is 0."""
    s = (len_sq(v[i], v[j]) + len_sq(v[j], v[k])) + len_sq(v[k], v[i])
    return F(0.0) if s == 0.0 else dot(n, n) / (s * s)


def edge_table(f):
    """{(lo, hi): {"n": owner count, "first": smallest corner id, "own": [(face, runs lo -> hi)]}}, (a, a) edges too."""
    table = {}
    for i, face in enumerate(f):
        for j in range(3):
            u, w = face[j], face[(j + 1) % 3]
            e = table.setdefault((min(u, w), max(u, w)), {"n": 0, "first": 3 * i + j, "own": []})
            e["n"] += 1
            e["own"].append((i, u < w))
    return table


def valence(f, nv, table=None, mask=None):
    """(deg (nv,) int64, border (nv,) bool, info): info = edges, open, nonmanifold, inconsistent, masked, deviation."""
    f = [tuple(int(x) for x in t) for t in np.asarray(f, dtype=np.int64).reshape(-1, 3).tolist()]
    table = edge_table(f) if table is None else table
    deg = np.zeros(nv, dtype=np.int64)
    border = np.zeros(nv, dtype=bool)
    info = dict(n_edges=0, n_open_edges=0, n_nonmanifold_edges=0, n_inconsistent_edges=0, n_masked_edges=0)
    for (lo, hi), e in table.items():
        if lo != hi:
            deg[lo] += 1
            deg[hi] += 1
            info["n_edges"] += 1
            info["n_inconsistent_edges"] += e["n"] == 2 and e["own"][0][1] == e["own"][1][1]
            info["n_masked_edges"] += mask is not None and bool(mask[lo] or mask[hi])
        if e["n"] != 2:
            border[lo] = border[hi] = True
        info["n_open_edges"] += e["n"] == 1
        info["n_nonmanifold_edges"] += e["n"] > 2
    ex = deg - np.where(border, 4, 6)
    info["deviation"] = int((ex * ex).sum())
    return deg, border, {k: int(x) for k, x in info.items()}


def one_pass(v, f, mask, cc2, qk2):
    """One pass over the faces f (a list of triples) as they are: {"candidates": [...], "flipped": [...], the four
    blocked counts, "info": the edge counts and the deviation}.  A candidate is a dict of lo, hi, c, d, fp, fm, g, prio."""
    nv = len(v)
    table = edge_table(f)
    deg, border, info = valence(f, nv, table, mask)
    ex = (deg - np.where(border, 4, 6)).tolist()
    out = {"candidates": [], "info": info, **{k: 0 for k in BLOCKS}}
    with np.errstate(all="ignore"):
        for (lo, hi), e in table.items():
            if lo == hi or e["n"] != 2 or e["own"][0][1] == e["own"][1][1]:                       # (a)
                continue
            fp, fm = (e["own"][0][0], e["own"][1][0]) if e["own"][0][1] else (e["own"][1][0], e["own"][0][0])
            if len(set(f[fp])) != 3 or len(set(f[fm])) != 3:                                      # (b)
                continue
            c, d = sum(f[fp]) - lo - hi, sum(f[fm]) - lo - hi
            if c == d:
                continue
            if mask is not None and (mask[lo] or mask[hi]):                                       # (c)
                continue
            g = 2 * (ex[lo] + ex[hi] - ex[c] - ex[d]) - 4                                         # (d)
            if not g > 0:
                continue
            if (min(c, d), max(c, d)) in table:                                                   # (e)
                out["blocked_existing"] += 1
                continue
            n0, n1 = cross(sub(v[hi], v[lo]), sub(v[c], v[lo])), cross(sub(v[lo], v[hi]), sub(v[d], v[hi]))
            m0, m1 = cross(sub(v[d], v[lo]), sub(v[c], v[lo])), cross(sub(v[c], v[hi]), sub(v[d], v[hi]))
            if not (dot(m0, n0) > 0.0 and dot(m0, n1) > 0.0 and dot(m1, n0) > 0.0 and dot(m1, n1) > 0.0):   # (f)
                out["blocked_normal"] += 1
                continue
            dn = dot(n0, n1)                                                                      # (g)
            if not (dn > 0.0 and dn * dn >= cc2 * (dot(n0, n0) * dot(n1, n1))):
                out["blocked_crease"] += 1
                continue
            t0, t1 = qk2 * quality(v, lo, hi, c, n0), qk2 * quality(v, hi, lo, d, n1)             # (h)
            q0, q1 = quality(v, lo, d, c, m0), quality(v, hi, c, d, m1)
            if not (q0 >= t0 and q0 >= t1 and q1 >= t0 and q1 >= t1):
                out["blocked_quality"] += 1
                continue
            prio = (min(g, GAIN_CAP) << 32) | (0xFFFFFFFF - e["first"])
            out["candidates"].append(dict(lo=lo, hi=hi, c=c, d=d, fp=fp, fm=fm, g=g, prio=prio))
    best = {}
    for k in out["candidates"]:
        for x in (k["lo"], k["hi"], k["c"], k["d"]):
            best[x] = max(best.get(x, 0), k["prio"])
    out["flipped"] = [k for k in out["candidates"] if all(best[x] == k["prio"] for x in (k["lo"], k["hi"], k["c"], k["d"]))]
    return out


def rewrite(f, flipped):
    """The faces after the flips, in place: F+ <- (lo, d, c), F- <- (hi, c, d)."""
    f = list(f)
    for k in flipped:
        f[k["fp"]] = (k["lo"], k["d"], k["c"])
        f[k["fm"]] = (k["hi"], k["c"], k["d"])
    return f


def predict_report(nv, nf, passes_run, converged, masked=False):
    """n_launches, bytes_uploaded and bytes_downloaded as the header states them."""
    if nv == 0 or nf == 0:
        return dict(n_launches=0, bytes_uploaded=0, bytes_downloaded=0)
    return dict(n_launches=PASS_LAUNCHES * passes_run + (0 if converged else STAT_LAUNCHES) + 2 * SMO.volume_launches(nf),
                bytes_uploaded=24 * nv + 12 * nf + (nv if masked else 0), bytes_downloaded=12 * nf + COUNTER_BYTES)


def flip(v, f, mask=None, crease_cos=crease_cos(), quality_keep=0.5, max_passes=50, trace=False):
    """(faces (nf, 3) int64, report[, one one_pass result per pass run])."""
    v = np.asarray(v, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    nv, nf = v.shape[0], f.shape[0]
    mask = None if mask is None else (np.asarray(mask).reshape(-1) != 0).tolist()
    cc2, qk2 = F(crease_cos) * F(crease_cos), F(quality_keep) * F(quality_keep)
    rep = {"n_vertices": nv, "n_faces": nf, "passes_run": 0, "converged": 0, "n_flips": 0,
           "flips_per_pass": [0] * SLOTS, "candidates_per_pass": [0] * SLOTS, **{k: 0 for k in BLOCKS}}
    cf = [tuple(int(x) for x in t) for t in f.tolist()]
    device = nv > 0 and nf > 0
    passes, first, last = [], None, None
    while device and rep["passes_run"] < int(max_passes):
        p = one_pass(v, cf, mask, cc2, qk2)
        passes.append(p)
        first = first or p["info"]
        slot = min(rep["passes_run"], SLOTS - 1)
        rep["passes_run"] += 1
        rep["candidates_per_pass"][slot] += len(p["candidates"])
        rep["flips_per_pass"][slot] += len(p["flipped"])
        rep["n_flips"] += len(p["flipped"])
        for k in BLOCKS:
            rep[k] += p[k]
        if not p["candidates"]:
            rep["converged"] = 1
            last = p["info"]
            break
        cf = rewrite(cf, p["flipped"])
    if device and not rep["converged"]:
        last = valence(cf, nv, None, mask)[2]
        first = first or last
    empty = valence([], nv)[2]                                          # no edge: every target is 6
    first, last = first or empty, last or empty
    out_f = np.array(cf, dtype=np.int64).reshape(-1, 3)
    for k in ("n_edges", "n_open_edges", "n_nonmanifold_edges", "n_inconsistent_edges", "n_masked_edges"):
        rep[k] = first[k]
    rep.update(deviation_before=first["deviation"], deviation_after=last["deviation"],
               volume_before=SMO.volume(v, f) if device else 0.0, volume_after=SMO.volume(v, out_f) if device else 0.0,
               **predict_report(nv, nf, rep["passes_run"], rep["converged"], mask is not None))
    return (out_f, rep, passes) if trace else (out_f, rep)
