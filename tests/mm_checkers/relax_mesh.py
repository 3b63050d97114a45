"""Plain numpy restatement of the mesh relaxation (include/mm_ccta.h, "mesh relaxation"): the yardstick for
csrc/mm_relax_kernels.hip and csrc/mm_relax.cpp.  Built on smooth_mesh.csr / smooth_mesh.step (the average) and
surface_distance.scan (the projection, unpruned); numpy's elementwise f64 operations are IEEE and unfused, so every line
is one rounding, in the header's order.

* `classify`: free, border and isolated vertices.
* `relax`: step 0, the iterations with their guard, the report; with `trace=True` also, per iteration, the candidates,
  the faces before it and the queries that did not move -- what `must_skip` needs -- and the vertices after it.
* `predict_report`: the report fields the data does not decide (launches, bytes, items).
* `must_skip`: per iteration, the items whose refreshed bound is >= the largest seed of their query block.  Stored
  minima only decrease, so the device skips at least these whatever the timing.
"""
import numpy as np

from . import smooth_mesh as SMO
from . import surface_distance as SD

SLACK_ULPS = 64.0                # tri_slack of csrc/mm_prune.h


def cross(u, w):
    """ab x ac with the component expressions of the degenerate test."""
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], axis=-1)


def face_normals(x, f):
    return cross(x[f[:, 1]] - x[f[:, 0]], x[f[:, 2]] - x[f[:, 0]])


def distinct(f):
    return (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])


def classify(f, nv, pinned=None):
    """(free, border, isolated) masks over the vertices."""
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    off, _, _ = SMO.csr(f, nv)
    isolated = np.diff(off) == 0
    border = np.zeros(nv, dtype=bool)
    if len(f):
        pairs = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
        edges, owners = np.unique(pairs, axis=0, return_counts=True)      # an (a, a) pair owns its edge too
        border[edges[owners != 2].reshape(-1)] = True
    mask = np.zeros(nv, dtype=bool) if pinned is None else np.asarray(pinned).reshape(-1) != 0
    return ~isolated & ~mask & ~border, border, isolated


def relax(v, f, rv=None, rf=None, iterations=5, lamb=0.5, pinned=None, trace=False):
    """(vertices, ref_face, report[, trace]).  rv is None: the mesh itself is the reference."""
    v = np.ascontiguousarray(np.asarray(v, dtype=np.float64).reshape(-1, 3))
    f = np.asarray(f, dtype=np.int64).reshape(-1, 3)
    if rv is None:
        rv, rf = v, f
    rv = np.asarray(rv, dtype=np.float64).reshape(-1, 3)
    rf = np.asarray(rf, dtype=np.int64).reshape(-1, 3)
    nv, nf = len(v), len(f)
    lamb = np.float64(lamb)
    free, border, isolated = classify(f, nv, pinned)
    off, nb, _ = SMO.csr(f, nv)
    idx = np.flatnonzero(free)
    x = v.copy()
    face = np.full(nv, -1, dtype=np.int64)
    init = 0.0
    steps = []
    reverted = 0
    if len(idx):
        assert len(rf), "a free vertex and no reference face"
        sq, fc, cl, _ = SD.scan(v[idx], rv, rf)
        hit = fc >= 0
        x[idx[hit]] = cl[hit]
        face[idx] = fc
        init = float(sq[hit].max()) if hit.any() else 0.0
        for _ in range(int(iterations)):
            with np.errstate(all="ignore"):                            # the sum of smooth_mesh.step, row by row
                acc = np.zeros_like(x)
                deg = np.diff(off)
                w = 1.0 / np.maximum(deg, 1).astype(np.float64)
                for k in range(int(deg.max())):
                    rows = np.flatnonzero(deg > k)
                    acc[rows] = acc[rows] + w[rows, None] * x[nb[off[rows] + k]]
                d = (acc - x)[idx]
                has = face[idx] >= 0
                t3 = rf[np.where(has, face[idx], 0)]
                n = cross(rv[t3[:, 1]] - rv[t3[:, 0]], rv[t3[:, 2]] - rv[t3[:, 0]])
                nn = SD.dot(n, n)
                ok = (nn > 0.0) & np.isfinite(nn)
                s = SD.dot(n, d) / np.where(ok, nn, 1.0)
                t = np.where(ok[:, None], d - n * s[:, None], d)
                c = x[idx] + lamb * t
            stays = ~has | ~np.isfinite(c).all(axis=1)
            cand = np.where(stays[:, None], x[idx], c)
            sq, fc, cl, _ = SD.scan(cand, rv, rf)
            stays = stays | (fc < 0)
            new = x.copy()
            new[idx[~stays]] = cl[~stays]
            with np.errstate(all="ignore"):
                m_old, m_new = face_normals(x, f), face_normals(new, f)
                bad = distinct(f) & (SD.dot(m_old, m_old) > 0.0) & ~(SD.dot(m_old, m_new) > 0.0)
            rev = np.zeros(nv, dtype=bool)
            rev[f[bad].reshape(-1)] = True
            rev &= free
            rev[idx[stays]] = True
            steps.append({"candidates": cand, "faces_before": face[idx].copy(), "stays": stays.copy()})
            keep = rev[idx]
            new[idx[keep]] = x[idx[keep]]
            face[idx[~keep]] = fc[~keep]
            reverted += int(rev.sum())
            x = new
            steps[-1]["vertices_after"] = x.copy()
    with np.errstate(all="ignore"):
        m_in, m_out = face_normals(v, f), face_normals(x, f)
        flipped = int((distinct(f) & (SD.dot(m_in, m_in) > 0.0) & (SD.dot(m_in, m_out) <= 0.0)).sum()) if nf else 0
        dd = x - v
        disp = (dd[:, 0] * dd[:, 0] + dd[:, 1] * dd[:, 1]) + dd[:, 2] * dd[:, 2]
    device = nv > 0 and nf > 0
    report = {"n_vertices": nv, "n_faces": nf, "n_ref_faces": len(rf), "n_free": int(free.sum()),
              "n_pinned": int(np.count_nonzero(pinned)) if pinned is not None else 0, "n_border": int(border.sum()),
              "n_isolated": int(isolated.sum()), "iterations_run": int(iterations), "n_reverted": reverted,
              "n_flipped_faces": flipped, "initial_distance_sq": init,
              "max_displacement_sq": float(disp.max()) if device else 0.0,
              "volume_before": SMO.volume(v, f) if device else 0.0, "volume_after": SMO.volume(x, f) if device else 0.0}
    face[~free] = -1
    return (x, face, report, steps) if trace else (x, face, report)


def predict_report(nv, nf, ref_nf, n_free, iterations, qpb=512, chunk=256):
    """n_launches, bytes_uploaded, bytes_downloaded and items_run + items_skipped as the header states them."""
    if nv == 0 or nf == 0:
        return dict(n_launches=0, bytes_uploaded=0, bytes_downloaded=0, items_total=0)
    up = SD.up256
    launches = 2 * SMO.volume_launches(nf) + 2
    bytes_up, bytes_down, items = up(12 * nf) + up(24 * nv), up(24 * nv) + 256, 0
    if n_free:
        nqb, nch = -(-n_free // qpb), -(-ref_nf // chunk)
        items = nqb * nch
        launches += SD.LAUNCHES + (1 if nch > 1 else 0) + 1 + 6 * iterations + (SMO.CSR_LAUNCHES if iterations else 0)
        bytes_up += up(96 * ref_nf) + up(24 * n_free) + up(4 * n_free) + up(16 * items) + up(48 * nch)
        bytes_down += up(8 * n_free)
    return dict(n_launches=launches, bytes_uploaded=bytes_up, bytes_downloaded=bytes_down,
                items_total=items * (1 + iterations))


def box_lb2(qlo, qhi, clo, chi):
    """box_lb2 with tri_slack of csrc/mm_prune.h, in its order of operations."""
    slack = SLACK_ULPS * np.finfo(np.float64).eps * max(np.abs(qlo).max(), np.abs(qhi).max(), np.abs(clo).max(),
                                                           np.abs(chi).max())
    s = 0.0
    for a in range(3):
        gap = max(0.0, max(qlo[a] - chi[a], clo[a] - qhi[a]) - slack)
        s += gap * gap
    return s * (1.0 - 1e-12)


def refreshed_items(plan, step, rv, rf):
    """[(q0, c0, lb2, top)] of one iteration: every (query block, chunk) item with its refreshed bound and the largest
    seed of its block.  plan: surface.tri_plan of the free vertices' input positions against the reference."""
    rv = np.asarray(rv, dtype=np.float64).reshape(-1, 3)
    rf = np.asarray(rf, dtype=np.int64).reshape(-1, 3)
    perm, qpb, ch = plan["query_perm"], plan["qpb"], plan["chunk"]
    cand, prev = step["candidates"][perm], step["faces_before"][perm]
    seed = np.full(len(cand), np.inf)
    for k in np.unique(prev[prev >= 0]):
        sel = prev == k
        t = rf[k]
        q = SD.closest_on_face(cand[sel], rv[t[0]], rv[t[1]], rv[t[2]], SD.face_kind(rv, t))[0]
        with np.errstate(all="ignore"):
            seed[sel] = SD.dist_sq(cand[sel], q)
    corners = rv[rf[plan["face_order"]]]                                   # (staged face, corner, xyz)
    out = []
    for q0 in range(0, len(cand), qpb):
        blk = cand[q0:q0 + qpb]
        qlo, qhi = blk.min(axis=0), blk.max(axis=0)
        top = seed[q0:q0 + qpb].max()
        for c0 in range(0, len(corners), ch):
            pts = corners[c0:c0 + ch].reshape(-1, 3)
            out.append((q0, c0, box_lb2(qlo, qhi, pts.min(axis=0), pts.max(axis=0)), top))
    return out


def must_skip(plan, steps, rv, rf):
    """Per iteration, the items the device skips whatever the timing: lb2 >= the largest seed of the block."""
    return [sum(1 for _, _, lb2, top in refreshed_items(plan, st, rv, rf) if lb2 >= top) for st in steps]
